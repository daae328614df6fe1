// The cell list on the unit sphere that gridgraph.hip (fixed-radius queries) and regrid.hip (k-nearest search) share.
//
// A uniform cell list over [-1, 1]^3, cells = clamp(floor(2 / R), 1, kCellCap) per axis (cell edge >= R unless the cap
// binds; then cells are larger than R and a query only visits more candidates).  Points are ordered by cell with one
// radix sort of UNIQUE 64-bit keys (cell << 32 | index) -- no stability assumption, no atomic decides an order -- and the
// cell starts are binary searches in the sorted keys.  A query visits the cells that [p - Rm, p + Rm] touches on every
// axis (Rm = R plus a margin far above any rounding of the cell function, which is monotone), so no pair the decision
// expression  (dx dx + dy dy) + dz dz <= r2  accepts is missed, whatever the cap does.  Everything sits in an anonymous
// namespace: each translation unit that includes this header gets its own copy.
#pragma once
#include "common.h"
#include <cmath>
#include <rocprim/device/device_radix_sort.hpp>

namespace {

constexpr int kThreads = 256;
// cells per axis at most: the dense cell_start table is (128^3 + 1) int32 = 8 MiB, L2-sized on MI355X, and the
// nu = 100 mesh at its default radius (2 / R = 252) still tests only a handful of candidates a query.
constexpr int kCellCap = 128;

inline int cells_for(double R) {
  const double q = 2.0 / R;
  if (!(q >= 1.0)) return 1;
  if (q >= (double)kCellCap) return kCellCap;
  return (int)std::floor(q);
}

inline int bits_for_host(uint64_t n) {  // smallest b >= 1 with (1 << b) >= n
  int b = 1;
  while ((uint64_t(1) << b) < n) ++b;
  return b;
}

// monotone in x; exactly +-1 (and anything outside, NaN included) lands in a valid cell
__device__ inline int cell_of(double x, int cells) {
  const double t = floor((x + 1.0) * 0.5 * (double)cells);
  if (!(t >= 0.0)) return 0;
  if (t >= (double)cells) return cells - 1;
  return (int)t;
}

struct CellList {
  int cells;
  const int32_t *cell_start;   // [cells^3 + 1]
  const double *spos;          // [n, 3] positions in cell order
  const int32_t *sidx;         // [n]    original index of sorted point k
};

__global__ __launch_bounds__(kThreads) void k_cell_keys(const double *__restrict__ pos, int64_t n, int cells,
                                                        uint64_t *__restrict__ keys) {
  const int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (i >= n) return;
  const uint64_t cx = (uint64_t)cell_of(pos[3 * i], cells), cy = (uint64_t)cell_of(pos[3 * i + 1], cells),
                 cz = (uint64_t)cell_of(pos[3 * i + 2], cells);
  keys[i] = (((cx * (uint64_t)cells + cy) * (uint64_t)cells + cz) << 32) | (uint64_t)i;
}

__device__ inline int64_t lower_bound_key(const uint64_t *a, int64_t n, uint64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void k_cell_start(const uint64_t *__restrict__ ks, int64_t n, int64_t ncells,
                                                         int32_t *__restrict__ cell_start) {
  const int64_t c = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (c > ncells) return;
  cell_start[c] = (int32_t)lower_bound_key(ks, n, (uint64_t)c << 32);
}

__global__ __launch_bounds__(kThreads) void k_cell_gather(const uint64_t *__restrict__ ks, const double *__restrict__ pos,
                                                          int64_t n, double *__restrict__ spos,
                                                          int32_t *__restrict__ sidx) {
  const int64_t k = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (k >= n) return;
  const int64_t i = (int64_t)(ks[k] & 0xffffffffull);
  spos[3 * k] = pos[3 * i];
  spos[3 * k + 1] = pos[3 * i + 1];
  spos[3 * k + 2] = pos[3 * i + 2];
  sidx[k] = (int32_t)i;
}

// f(original index, d2) for every listed point s with d2 = (dx dx + dy dy) + dz dz <= r2, d = p - s.  Cells of one
// (cx, cy) column are contiguous in z, so a query walks at most 3 x 3 (rarely 4 x 4) ranges.
template <class F>
__device__ inline void for_each_within_d2(const CellList &L, double px, double py, double pz, double rm, double r2,
                                          F &&f) {
  const int n = L.cells;
  const int x0 = cell_of(px - rm, n), x1 = cell_of(px + rm, n);
  const int y0 = cell_of(py - rm, n), y1 = cell_of(py + rm, n);
  const int z0 = cell_of(pz - rm, n), z1 = cell_of(pz + rm, n);
  for (int cx = x0; cx <= x1; ++cx)
    for (int cy = y0; cy <= y1; ++cy) {
      const int64_t base = ((int64_t)cx * n + cy) * n;
      const int32_t k1 = L.cell_start[base + z1 + 1];
      for (int32_t k = L.cell_start[base + z0]; k < k1; ++k) {
        const double dx = px - L.spos[3 * (int64_t)k], dy = py - L.spos[3 * (int64_t)k + 1],
                     dz = pz - L.spos[3 * (int64_t)k + 2];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 <= r2) f(L.sidx[k], d2);
      }
    }
}

// the same walk and the same decision for callers that only want the index
template <class F>
__device__ inline void for_each_within(const CellList &L, double px, double py, double pz, double rm, double r2, F &&f) {
  for_each_within_d2(L, px, py, pz, rm, r2, [&](int32_t j, double) { f(j); });
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }
inline size_t at_least_one(int64_t n) { return (size_t)(n > 0 ? n : 1); }

struct CellWs {                     // the cell list of n points, sized for any radius
  size_t keys_in, keys_out, temp, temp_bytes, cell_start, spos, sidx, end;
};

int cell_ws(int64_t n, CellWs *W) {
  size_t off = 0;
  W->keys_in = off;  off = gwen_align_up(off + sizeof(uint64_t) * at_least_one(n), 256);
  W->keys_out = off; off = gwen_align_up(off + sizeof(uint64_t) * at_least_one(n), 256);
  size_t tb = 0;
  hipError_t e = rocprim::radix_sort_keys(nullptr, tb, (uint64_t *)nullptr, (uint64_t *)nullptr, at_least_one(n), 0u, 64u);
  if (e != hipSuccess) return (int)e;
  W->temp = off; W->temp_bytes = tb; off = gwen_align_up(off + tb, 256);
  W->cell_start = off; off = gwen_align_up(off + sizeof(int32_t) * ((size_t)kCellCap * kCellCap * kCellCap + 1), 256);
  W->spos = off; off = gwen_align_up(off + sizeof(double) * 3 * at_least_one(n), 256);
  W->sidx = off; off = gwen_align_up(off + sizeof(int32_t) * at_least_one(n), 256);
  W->end = off;
  return GWEN_OK;
}

inline CellList cell_view(const CellWs &W, const char *ws, int cells) {
  return CellList{cells, reinterpret_cast<const int32_t *>(ws + W.cell_start),
                  reinterpret_cast<const double *>(ws + W.spos), reinterpret_cast<const int32_t *>(ws + W.sidx)};
}

// keys -> sort -> cell starts -> positions in cell order; everything lands in the workspace
int cell_build(const double *pos, int64_t n, int cells, const CellWs &W, char *ws, hipStream_t stream) {
  uint64_t *keys_in = reinterpret_cast<uint64_t *>(ws + W.keys_in);
  uint64_t *keys_out = reinterpret_cast<uint64_t *>(ws + W.keys_out);
  const int64_t ncells = (int64_t)cells * cells * cells;
  if (n > 0) {
    k_cell_keys<<<blocks_for(n), kThreads, 0, stream>>>(pos, n, cells, keys_in);
    GWEN_LAUNCH_CHECK();
    size_t tb = W.temp_bytes;
    GWEN_HIP_CHECK(rocprim::radix_sort_keys(ws + W.temp, tb, keys_in, keys_out, (size_t)n, 0u,
                                            (unsigned)(32 + bits_for_host((uint64_t)ncells + 1)), stream));
  }
  k_cell_start<<<blocks_for(ncells + 1), kThreads, 0, stream>>>(keys_out, n, ncells,
                                                                reinterpret_cast<int32_t *>(ws + W.cell_start));
  GWEN_LAUNCH_CHECK();
  if (n > 0) {
    k_cell_gather<<<blocks_for(n), kThreads, 0, stream>>>(keys_out, pos, n, reinterpret_cast<double *>(ws + W.spos),
                                                          reinterpret_cast<int32_t *>(ws + W.sidx));
    GWEN_LAUNCH_CHECK();
  }
  return GWEN_OK;
}

inline bool radius_ok(double r) { return r > 0.0 && std::isfinite(r); }
inline double margin(double r) { return r * 1.000001 + 1e-12; }
constexpr int64_t kIndexLimit = (int64_t(1) << 31) - 1;

}  // namespace
