// Regridding -- the exact k nearest source points of every target point on the unit sphere, and interpolation weights.
//
// BUILD-DEFINED, PARITY UNPINNED: the reference moves no field between point sets; the contract is
// this build's own (include/gwen_hip.h, "Regridding"; DESIGN.md, "Regridding") and is restated in numpy in
// tests/regrid_ref.py.
//
// The search runs through the cell list of cell_list.h (shared with gridgraph.hip).  One thread per target row keeps its
// K best candidates in registers by insertion while for_each_within_d2 walks the cells for a radius R:
//     candidate      a listed source with  d2 = (dx dx + dy dy) + dz dz <= r2  on dst - src, fp64, this association (the
//                    library is built with -ffp-contract=off: numpy computes the same bits);
//     order          ascending (d2, reported source index), lexicographic: the lowest index wins every tie, whatever
//                    order the cells are visited in -- insertion compares the pair, never the arrival order.
// A row that finds at least K candidates within R is FINAL: everything the walk rejected has d2 > R R, farther than
// everything the row kept.  A row that found fewer is flagged, the flagged row ids are compacted (flag -> exclusive scan
// -> scatter, in row order) and their number lands in next_count; the host reads that one number, doubles R, and calls
// again for those rows only, on a cell list rebuilt for the new radius.  A call whose radius reaches max_distance (r2 =
// D D, every candidate seen) or 2 (one cell, the whole sphere) finishes every row it is given, so the loop ends.  The
// result does not depend on the starting radius: a final row holds the K least pairs of ALL candidates either way.
//
// A source mask is applied BEFORE the cell list: the caller lists the unmasked sources only and passes their original
// indices as src_ids, which is what a row reports and what breaks ties.
//
// Accepted cost: the nlon points of a pole row of a lat-lon source coincide, so they share one cell and a target next
// to the pole walks all of them (a serial walk of nlon candidates in a handful of threads).  No atomics anywhere: two
// builds are bitwise equal.
#include "cell_list.h"
#include <rocprim/device/device_scan.hpp>

namespace {

constexpr int kMaxK = 8;
constexpr double kCoincident2 = 1e-24;      // a target with nearest d2 <= this sits ON that source

template <int K>
__global__ __launch_bounds__(kThreads) void k_knn(CellList L, const int32_t *__restrict__ ids,
                                                  const double *__restrict__ dpos, int64_t nd,
                                                  const int32_t *__restrict__ rows, int64_t nrows, double rm, double r2,
                                                  int last, int32_t *__restrict__ idx, double *__restrict__ d2out,
                                                  int32_t *__restrict__ count, int32_t *__restrict__ flag) {
  const int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (i >= nrows) return;
  const int64_t t = rows ? (int64_t)rows[i] : i;
  if (t < 0 || t >= nd) { flag[i] = 0; return; }                      // never out of range
  const double px = dpos[3 * t], py = dpos[3 * t + 1], pz = dpos[3 * t + 2];
  double bd[K];
  int32_t bi[K];
#pragma unroll
  for (int s = 0; s < K; ++s) { bd[s] = INFINITY; bi[s] = INT32_MAX; }
  int32_t c = 0;
  for_each_within_d2(L, px, py, pz, rm, r2, [&](int32_t j, double d) {
    const int32_t id = ids ? ids[j] : j;
    ++c;
    if (d < bd[K - 1] || (d == bd[K - 1] && id < bi[K - 1])) {
      bd[K - 1] = d; bi[K - 1] = id;
#pragma unroll
      for (int s = K - 1; s > 0; --s) {
        const bool lt = bd[s] < bd[s - 1] || (bd[s] == bd[s - 1] && bi[s] < bi[s - 1]);
        const double td = lt ? bd[s - 1] : bd[s];
        const int32_t ti = lt ? bi[s - 1] : bi[s];
        bd[s - 1] = lt ? bd[s] : bd[s - 1]; bi[s - 1] = lt ? bi[s] : bi[s - 1];
        bd[s] = td; bi[s] = ti;
      }
    }
  });
  const bool done = last || c >= K;
  flag[i] = done ? 0 : 1;
  if (!done) return;
  const int32_t n = c < K ? c : K;
#pragma unroll
  for (int s = 0; s < K; ++s) {
    idx[t * K + s] = s < n ? bi[s] : -1;
    d2out[t * K + s] = s < n ? bd[s] : (double)INFINITY;
  }
  count[t] = n;
}

// next_rows = the flagged rows in row order; next_count[0] = their number
__global__ __launch_bounds__(kThreads) void k_knn_compact(const int32_t *__restrict__ flag, const int32_t *__restrict__ off,
                                                          const int32_t *__restrict__ rows, int64_t nrows,
                                                          int32_t *__restrict__ next_rows,
                                                          int32_t *__restrict__ next_count) {
  const int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (i >= nrows) return;
  const int32_t o = off[i];
  if (flag[i] && o >= 0 && o < nrows) next_rows[o] = rows ? rows[i] : (int32_t)i;
  if (i == nrows - 1) next_count[0] = o + flag[i];
}

__device__ inline double idw_term(double d2, double power) {
  if (power == 1.0) return 1.0 / sqrt(d2);
  if (power == 2.0) return 1.0 / d2;
  return pow(sqrt(d2), -power);
}

// one thread per target: fp64 weights over the row's stored order, rounded to fp32
__global__ __launch_bounds__(kThreads) void k_knn_weights(const double *__restrict__ d2, const int32_t *__restrict__ count,
                                                          int64_t nd, int k, int method, double power,
                                                          float *__restrict__ w, int32_t *__restrict__ entries) {
  const int64_t t = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (t >= nd) return;
  int32_t c = count[t];
  c = c < 0 ? 0 : (c > k ? k : c);
  const double *row = d2 + t * k;
  float *out = w + t * k;
  const bool single = c > 0 && (method == GWEN_REGRID_NEAREST || row[0] <= kCoincident2);
  if (single) c = 1;
  double sum = 0.0;
  if (!single)
    for (int s = 0; s < c; ++s) sum += idw_term(row[s], power);
  for (int s = 0; s < k; ++s) out[s] = s >= c ? 0.0f : single ? 1.0f : (float)(idw_term(row[s], power) / sum);
  entries[t] = c;
}

struct KnnWs {
  CellWs cell;
  size_t flag, off, scan, scan_bytes, total;
};

int knn_ws(int64_t ns, int64_t nd, KnnWs *W) {
  int rc = cell_ws(ns, &W->cell);
  if (rc != GWEN_OK) return rc;
  size_t off = W->cell.end;
  W->flag = off; off = gwen_align_up(off + sizeof(int32_t) * at_least_one(nd), 256);
  W->off = off;  off = gwen_align_up(off + sizeof(int32_t) * at_least_one(nd), 256);
  size_t tb = 0;
  hipError_t e = rocprim::exclusive_scan(nullptr, tb, (int32_t *)nullptr, (int32_t *)nullptr, int32_t(0),
                                         at_least_one(nd), rocprim::plus<int32_t>());
  if (e != hipSuccess) return (int)e;
  W->scan = off; W->scan_bytes = tb; off = gwen_align_up(off + tb, 256);
  W->total = off;
  return GWEN_OK;
}

template <int K>
int knn_launch(const CellList &L, const int32_t *ids, const double *dpos, int64_t nd, const int32_t *rows, int64_t nrows,
               double rm, double r2, int last, int32_t *idx, double *d2, int32_t *count, int32_t *flag,
               hipStream_t stream) {
  k_knn<K><<<blocks_for(nrows), kThreads, 0, stream>>>(L, ids, dpos, nd, rows, nrows, rm, r2, last, idx, d2, count, flag);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

inline bool k_ok(int k) { return k >= 1 && k <= kMaxK; }

}  // namespace

extern "C" int gwen_knn_workspace_bytes(int64_t num_src, int64_t num_dst, size_t *bytes) {
  if (!bytes || num_src < 0 || num_dst < 0) return GWEN_EINVAL;
  if (num_src >= kIndexLimit || num_dst >= kIndexLimit) return GWEN_ERANGE;
  KnnWs W;
  int rc = knn_ws(num_src, num_dst, &W);
  if (rc != GWEN_OK) return rc;
  *bytes = W.total;
  return GWEN_OK;
}

extern "C" int gwen_knn_query(const double *src_pos, const int32_t *src_ids, int64_t num_src, const double *dst_pos,
                              int64_t num_dst, const int32_t *rows, int64_t num_rows, int k, double radius,
                              double max_distance, int32_t *idx, double *d2, int32_t *count, int32_t *next_rows,
                              int32_t *next_count, void *workspace, size_t workspace_bytes, gwen_stream_t stream_) {
  if (num_src < 0 || num_dst < 0 || num_rows < 0 || num_rows > num_dst || !k_ok(k) || !radius_ok(radius)) return GWEN_EINVAL;
  if (!(max_distance == max_distance) || std::isinf(max_distance)) return GWEN_EINVAL;      // NaN, +-inf
  if (!rows && num_rows != num_dst) return GWEN_EINVAL;
  if (num_src >= kIndexLimit || num_dst >= kIndexLimit || num_dst * k >= kIndexLimit) return GWEN_ERANGE;
  if (num_rows == 0) return GWEN_OK;
  if (!dst_pos || !idx || !d2 || !count || !next_rows || !next_count || (num_src > 0 && !src_pos)) return GWEN_EINVAL;
  KnnWs W;
  int rc = knn_ws(num_src, num_dst, &W);
  if (rc != GWEN_OK) return rc;
  if (!workspace || workspace_bytes < W.total) return GWEN_ENOSPACE;
  hipStream_t stream = gwen_stream(stream_);
  char *ws = static_cast<char *>(workspace);
  // the last call of a row: the radius has reached max_distance (every candidate lies within D) or the whole sphere
  const bool bounded = max_distance >= 0.0;
  const int last = (bounded && radius >= max_distance) || radius >= 2.0;
  double walk = radius, r2 = radius * radius;
  if (last) {
    walk = bounded && max_distance < 2.0 ? max_distance : 2.0;
    r2 = bounded ? max_distance * max_distance : (double)INFINITY;
  }
  if (!(walk > 0.0)) walk = 1e-300;                                    // max_distance == 0: coincident sources only
  const int cells = cells_for(walk);
  rc = cell_build(src_pos, num_src, cells, W.cell, ws, stream);
  if (rc != GWEN_OK) return rc;
  const CellList L = cell_view(W.cell, ws, cells);
  int32_t *flag = reinterpret_cast<int32_t *>(ws + W.flag), *off = reinterpret_cast<int32_t *>(ws + W.off);
  const double rm = margin(walk);
#define GWEN_KNN_CASE(K) \
  case K: rc = knn_launch<K>(L, src_ids, dst_pos, num_dst, rows, num_rows, rm, r2, last, idx, d2, count, flag, stream); break;
  switch (k) {
    GWEN_KNN_CASE(1) GWEN_KNN_CASE(2) GWEN_KNN_CASE(3) GWEN_KNN_CASE(4)
    GWEN_KNN_CASE(5) GWEN_KNN_CASE(6) GWEN_KNN_CASE(7) GWEN_KNN_CASE(8)
    default: return GWEN_EINVAL;
  }
#undef GWEN_KNN_CASE
  if (rc != GWEN_OK) return rc;
  size_t tb = W.scan_bytes;
  GWEN_HIP_CHECK(rocprim::exclusive_scan(ws + W.scan, tb, flag, off, int32_t(0), (size_t)num_rows,
                                         rocprim::plus<int32_t>(), stream));
  k_knn_compact<<<blocks_for(num_rows), kThreads, 0, stream>>>(flag, off, rows, num_rows, next_rows, next_count);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

extern "C" int gwen_knn_weights(const double *d2, const int32_t *count, int64_t num_dst, int k, int method,
                                double power, float *weights, int32_t *entries, gwen_stream_t stream_) {
  if (num_dst < 0 || !k_ok(k) || (method != GWEN_REGRID_NEAREST && method != GWEN_REGRID_IDW)) return GWEN_EINVAL;
  if (method == GWEN_REGRID_IDW && !(power > 0.0 && std::isfinite(power))) return GWEN_EINVAL;
  if (num_dst >= kIndexLimit || num_dst * k >= kIndexLimit) return GWEN_ERANGE;
  if (num_dst == 0) return GWEN_OK;
  if (!d2 || !count || !weights || !entries) return GWEN_EINVAL;
  k_knn_weights<<<blocks_for(num_dst), kThreads, 0, gwen_stream(stream_)>>>(d2, count, num_dst, k, method, power,
                                                                            weights, entries);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}
