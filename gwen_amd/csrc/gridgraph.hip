// Grid graphs -- the grid <-> mesh graphs of the forecaster for ARBITRARY grid points, built on the device.
//
// BUILD-DEFINED, PARITY UNPINNED: the reference has no grid <-> mesh graphs at all, so there is
// nothing in it to compare with; the contracts below are this build's own ("Grid graphs") and are
// restated in numpy in tests/gridgraph_ref.py.
//
// One piece of machinery: a fixed-radius neighbour query on the unit sphere through a uniform cell list over
// [-1, 1]^3, cells = clamp(floor(2 / R), 1, kCellCap) per axis (cell edge >= R unless the cap binds; then cells are
// larger than R and a query only visits more candidates).  Points are ordered by cell with one radix sort of
// UNIQUE 64-bit keys (cell << 32 | index) -- the pattern of prep.hip: no stability assumption, no atomic decides an
// order -- and the cell starts are binary searches in the sorted keys.  A query visits the cells that
// [p - Rm, p + Rm] touches on every axis (Rm = R plus a margin far above any rounding of the cell function, which
// is monotone), so no pair the decision expression accepts is missed, whatever the cap does.
//
// Two products:
//   radius edges      every (s, d) with  (dx dx + dy dy) + dz dz <= R R  on  d_pos - s_pos,  fp64, exactly this
//                     association (the library is built with -ffp-contract=off, so a numpy restatement decides
//                     every pair identically); count -> exclusive scan (64-bit) -> fill -> one radix sort of the
//                     unique keys (d << 32 | s): the list comes out sorted by (d, s), and rowptr is read off the
//                     sorted keys.  The LARGER set asks (one thread per point), the smaller is listed: on a lat-lon
//                     grid over a mesh a million threads find <= 4 nodes each, where one thread per mesh node would
//                     leave a pole node's thread walking thousands of coincident points alone.
//   containing faces  for a point p the LOWEST face id (a, b, c), among the faces whose centre is within R of p,
//                     with det(p,b,c), det(p,c,a), det(p,a,b) all >= -1e-12, and the three determinants over
//                     their sum as barycentric weights.
// No atomics anywhere: two runs are bitwise equal.  Coordinates are fp64 (a once-per-grid pass).
#include "cell_list.h"
#include <rocprim/device/device_scan.hpp>

namespace {

constexpr double kFaceTol = -1e-12;

// The QUERYING set is the larger of the two (one thread per point, its hits are the few listed points near it); the
// listed set is the smaller.  Which side asks does not change a decision: (-dx)(-dx) is dx dx to the last bit.
__global__ __launch_bounds__(kThreads) void k_radius_count(CellList L, const double *__restrict__ qpos, int64_t nq,
                                                           double rm, double r2, int64_t *__restrict__ cnt) {
  const int64_t q = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (q > nq) return;
  int64_t c = 0;
  if (q < nq) for_each_within(L, qpos[3 * q], qpos[3 * q + 1], qpos[3 * q + 2], rm, r2, [&](int32_t) { ++c; });
  cnt[q] = c;                                   // cnt[nq] = 0: the scan's last entry is the total
}

__global__ void k_total_out(const int64_t *__restrict__ off, int64_t nq, int64_t *__restrict__ total) {
  total[0] = off[nq];
}

// key = (d << 32) | s at the query's own slots; the sort that follows orders the list by (d, s)
__global__ __launch_bounds__(kThreads) void k_radius_fill(CellList L, const double *__restrict__ qpos, int64_t nq,
                                                          int query_is_src, double rm, double r2,
                                                          const int64_t *__restrict__ off, int64_t E,
                                                          uint64_t *__restrict__ keys) {
  const int64_t q = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (q >= nq) return;
  int64_t slot = off[q];
  for_each_within(L, qpos[3 * q], qpos[3 * q + 1], qpos[3 * q + 2], rm, r2, [&](int32_t j) {
    const uint64_t s = query_is_src ? (uint64_t)q : (uint64_t)(uint32_t)j, d = query_is_src ? (uint64_t)(uint32_t)j : (uint64_t)q;
    if (slot >= 0 && slot < E) keys[slot] = (d << 32) | s;                     // never out of range
    ++slot;
  });
}

__global__ __launch_bounds__(kThreads) void k_edges_out(const uint64_t *__restrict__ ks, int64_t E,
                                                        int64_t *__restrict__ edge_index) {
  const int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (i >= E) return;
  const uint64_t k = ks[i];
  edge_index[i] = (int64_t)(k & 0xffffffffull);
  edge_index[E + i] = (int64_t)(k >> 32);
}

// rowptr[r] = number of edges with target < r, from the sorted keys
__global__ __launch_bounds__(kThreads) void k_rowptr_out(const uint64_t *__restrict__ ks, int64_t E, int64_t nd,
                                                         int32_t *__restrict__ rowptr) {
  const int64_t r = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (r > nd) return;
  rowptr[r] = (int32_t)lower_bound_key(ks, E, (uint64_t)r << 32);
}

// u . (v x w), in this association
__device__ inline double det3(const double *u, const double *v, const double *w) {
  return (u[0] * (v[1] * w[2] - v[2] * w[1]) + u[1] * (v[2] * w[0] - v[0] * w[2])) + u[2] * (v[0] * w[1] - v[1] * w[0]);
}

__global__ __launch_bounds__(kThreads) void k_containing_faces(CellList L, const double *__restrict__ points, int64_t n,
                                                               double rm, double r2, const double *__restrict__ mesh_pos,
                                                               int64_t num_nodes, const int64_t *__restrict__ faces,
                                                               int32_t *__restrict__ face, double *__restrict__ w) {
  const int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (i >= n) return;
  const double p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
  int32_t best = -1;
  double b0 = 0.0, b1 = 0.0, b2 = 0.0;
  for_each_within(L, p[0], p[1], p[2], rm, r2, [&](int32_t f) {
    if (best >= 0 && f >= best) return;                         // the lowest face id wins
    const int64_t ia = faces[3 * (int64_t)f], ib = faces[3 * (int64_t)f + 1], ic = faces[3 * (int64_t)f + 2];
    if (ia < 0 || ia >= num_nodes || ib < 0 || ib >= num_nodes || ic < 0 || ic >= num_nodes) return;
    const double *a = mesh_pos + 3 * ia, *b = mesh_pos + 3 * ib, *c = mesh_pos + 3 * ic;
    const double d0 = det3(p, b, c), d1 = det3(p, c, a), d2 = det3(p, a, b);
    if (d0 >= kFaceTol && d1 >= kFaceTol && d2 >= kFaceTol) { best = f; b0 = d0; b1 = d1; b2 = d2; }
  });
  face[i] = best;
  const double s = (b0 + b1) + b2;
  w[3 * i] = best >= 0 ? b0 / s : 0.0;
  w[3 * i + 1] = best >= 0 ? b1 / s : 0.0;
  w[3 * i + 2] = best >= 0 ? b2 / s : 0.0;
}

struct RadiusWs {
  CellWs cell;
  size_t cnt, rp64, scan, scan_bytes, total;
};

// the source set queries when it is the larger one (a lat-lon grid over a mesh: a million short queries, and the pole
// rows' coincident points each ask for themselves); a function of the two sizes alone, so count and fill agree
inline bool query_is_src(int64_t ns, int64_t nd) { return ns > nd; }

int radius_ws(int64_t ns, int64_t nd, RadiusWs *W) {
  const int64_t nl = query_is_src(ns, nd) ? nd : ns, nq = query_is_src(ns, nd) ? ns : nd;      // listed, querying
  int rc = cell_ws(nl, &W->cell);
  if (rc != GWEN_OK) return rc;
  size_t off = W->cell.end;
  W->cnt = off;  off = gwen_align_up(off + sizeof(int64_t) * (size_t)(nq + 1), 256);
  W->rp64 = off; off = gwen_align_up(off + sizeof(int64_t) * (size_t)(nq + 1), 256);
  size_t tb = 0;
  hipError_t e = rocprim::exclusive_scan(nullptr, tb, (int64_t *)nullptr, (int64_t *)nullptr, int64_t(0),
                                         (size_t)(nq + 1), rocprim::plus<int64_t>());
  if (e != hipSuccess) return (int)e;
  W->scan = off; W->scan_bytes = tb; off = gwen_align_up(off + tb, 256);
  W->total = off;
  return GWEN_OK;
}

struct FillWs {
  size_t keys_in, keys_out, temp, temp_bytes, total;
};

int fill_ws(int64_t E, FillWs *W) {
  size_t off = 0;
  W->keys_in = off;  off = gwen_align_up(off + sizeof(uint64_t) * at_least_one(E), 256);
  W->keys_out = off; off = gwen_align_up(off + sizeof(uint64_t) * at_least_one(E), 256);
  size_t tb = 0;
  hipError_t e = rocprim::radix_sort_keys(nullptr, tb, (uint64_t *)nullptr, (uint64_t *)nullptr, at_least_one(E), 0u, 64u);
  if (e != hipSuccess) return (int)e;
  W->temp = off; W->temp_bytes = tb; off = gwen_align_up(off + tb, 256);
  W->total = off;
  return GWEN_OK;
}

}  // namespace

extern "C" int gwen_gridgraph_cells(double radius) { return radius_ok(radius) ? cells_for(radius) : GWEN_EINVAL; }

extern "C" int gwen_radius_edges_workspace_bytes(int64_t num_src, int64_t num_dst, size_t *bytes) {
  if (!bytes || num_src < 0 || num_dst < 0) return GWEN_EINVAL;
  if (num_src >= kIndexLimit || num_dst >= kIndexLimit) return GWEN_ERANGE;
  RadiusWs W;
  int rc = radius_ws(num_src, num_dst, &W);
  if (rc != GWEN_OK) return rc;
  *bytes = W.total;
  return GWEN_OK;
}

extern "C" int gwen_radius_edges_count(const double *src_pos, int64_t num_src, const double *dst_pos, int64_t num_dst,
                                       double radius, int64_t *total, void *workspace, size_t workspace_bytes,
                                       gwen_stream_t stream_) {
  if (num_src < 0 || num_dst < 0 || !radius_ok(radius) || !total) return GWEN_EINVAL;
  if ((num_src > 0 && !src_pos) || (num_dst > 0 && !dst_pos)) return GWEN_EINVAL;
  if (num_src >= kIndexLimit || num_dst >= kIndexLimit) return GWEN_ERANGE;
  RadiusWs W;
  int rc = radius_ws(num_src, num_dst, &W);
  if (rc != GWEN_OK) return rc;
  if (!workspace || workspace_bytes < W.total) return GWEN_ENOSPACE;
  hipStream_t stream = gwen_stream(stream_);
  char *ws = static_cast<char *>(workspace);
  const bool by_src = query_is_src(num_src, num_dst);
  const double *lpos = by_src ? dst_pos : src_pos, *qpos = by_src ? src_pos : dst_pos;
  const int64_t nl = by_src ? num_dst : num_src, nq = by_src ? num_src : num_dst;
  const int cells = cells_for(radius);
  rc = cell_build(lpos, nl, cells, W.cell, ws, stream);
  if (rc != GWEN_OK) return rc;
  int64_t *cnt = reinterpret_cast<int64_t *>(ws + W.cnt), *off = reinterpret_cast<int64_t *>(ws + W.rp64);
  k_radius_count<<<blocks_for(nq + 1), kThreads, 0, stream>>>(cell_view(W.cell, ws, cells), qpos, nq, margin(radius),
                                                              radius * radius, cnt);
  GWEN_LAUNCH_CHECK();
  size_t tb = W.scan_bytes;
  GWEN_HIP_CHECK(rocprim::exclusive_scan(ws + W.scan, tb, cnt, off, int64_t(0), (size_t)(nq + 1),
                                         rocprim::plus<int64_t>(), stream));
  k_total_out<<<1, 1, 0, stream>>>(off, nq, total);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

extern "C" int gwen_radius_edges_fill_workspace_bytes(int64_t E, size_t *bytes) {
  if (!bytes || E < 0) return GWEN_EINVAL;
  if (E >= kIndexLimit) return GWEN_ERANGE;
  FillWs W;
  int rc = fill_ws(E, &W);
  if (rc != GWEN_OK) return rc;
  *bytes = W.total;
  return GWEN_OK;
}

extern "C" int gwen_radius_edges_fill(const double *src_pos, int64_t num_src, const double *dst_pos, int64_t num_dst,
                                      double radius, int64_t E, int32_t *rowptr, int64_t *edge_index,
                                      const void *workspace, size_t workspace_bytes, void *sort_workspace,
                                      size_t sort_workspace_bytes, gwen_stream_t stream_) {
  if (num_src < 0 || num_dst < 0 || E < 0 || !radius_ok(radius) || !rowptr) return GWEN_EINVAL;
  if (num_src >= kIndexLimit || num_dst >= kIndexLimit || E >= kIndexLimit) return GWEN_ERANGE;
  if (E > 0 && (!src_pos || !dst_pos || !edge_index || num_dst == 0 || num_src == 0)) return GWEN_EINVAL;
  RadiusWs W;
  int rc = radius_ws(num_src, num_dst, &W);
  if (rc != GWEN_OK) return rc;
  FillWs F;
  rc = fill_ws(E, &F);
  if (rc != GWEN_OK) return rc;
  if (!sort_workspace || sort_workspace_bytes < F.total) return GWEN_ENOSPACE;
  if (E > 0 && (!workspace || workspace_bytes < W.total)) return GWEN_ENOSPACE;
  hipStream_t stream = gwen_stream(stream_);
  const char *ws = static_cast<const char *>(workspace);
  char *sw = static_cast<char *>(sort_workspace);
  uint64_t *keys_in = reinterpret_cast<uint64_t *>(sw + F.keys_in), *keys_out = reinterpret_cast<uint64_t *>(sw + F.keys_out);
  if (E > 0) {
    const bool by_src = query_is_src(num_src, num_dst);
    // an E larger than the count's total must not leave a slot unwritten: such keys are all-ones and sort last
    GWEN_HIP_CHECK(hipMemsetAsync(keys_in, 0xff, sizeof(uint64_t) * (size_t)E, stream));
    k_radius_fill<<<blocks_for(by_src ? num_src : num_dst), kThreads, 0, stream>>>(
        cell_view(W.cell, ws, cells_for(radius)), by_src ? src_pos : dst_pos, by_src ? num_src : num_dst, (int)by_src,
        margin(radius), radius * radius, reinterpret_cast<const int64_t *>(ws + W.rp64), E, keys_in);
    GWEN_LAUNCH_CHECK();
    size_t tb = F.temp_bytes;
    GWEN_HIP_CHECK(rocprim::radix_sort_keys(sw + F.temp, tb, keys_in, keys_out, (size_t)E, 0u, 64u, stream));
    k_edges_out<<<blocks_for(E), kThreads, 0, stream>>>(keys_out, E, edge_index);
    GWEN_LAUNCH_CHECK();
  }
  k_rowptr_out<<<blocks_for(num_dst + 1), kThreads, 0, stream>>>(keys_out, E, num_dst, rowptr);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

extern "C" int gwen_containing_faces_workspace_bytes(int64_t num_faces, size_t *bytes) {
  if (!bytes || num_faces < 0) return GWEN_EINVAL;
  if (num_faces >= kIndexLimit) return GWEN_ERANGE;
  CellWs W;
  int rc = cell_ws(num_faces, &W);
  if (rc != GWEN_OK) return rc;
  *bytes = W.end;
  return GWEN_OK;
}

extern "C" int gwen_containing_faces(const double *points, int64_t n, const double *mesh_pos, int64_t num_nodes,
                                     const int64_t *faces, const double *centres, int64_t num_faces, double radius,
                                     int32_t *face, double *weights, void *workspace, size_t workspace_bytes,
                                     gwen_stream_t stream_) {
  if (n < 0 || num_nodes < 0 || num_faces < 0 || !radius_ok(radius)) return GWEN_EINVAL;
  if (n >= kIndexLimit || num_nodes >= kIndexLimit || num_faces >= kIndexLimit) return GWEN_ERANGE;
  if (n == 0) return GWEN_OK;
  if (!points || !face || !weights || (num_faces > 0 && (!mesh_pos || !faces || !centres))) return GWEN_EINVAL;
  CellWs W;
  int rc = cell_ws(num_faces, &W);
  if (rc != GWEN_OK) return rc;
  if (!workspace || workspace_bytes < W.end) return GWEN_ENOSPACE;
  hipStream_t stream = gwen_stream(stream_);
  char *ws = static_cast<char *>(workspace);
  const int cells = cells_for(radius);
  rc = cell_build(centres, num_faces, cells, W, ws, stream);
  if (rc != GWEN_OK) return rc;
  k_containing_faces<<<blocks_for(n), kThreads, 0, stream>>>(cell_view(W, ws, cells), points, n, margin(radius),
                                                             radius * radius, mesh_pos, num_nodes, faces, face, weights);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}
