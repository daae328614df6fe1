// Conservative regridding -- the area of intersection of two convex spherical polygons for every candidate pair of
// cells, and the first-order conservative weights from those areas.
//
// BUILD-DEFINED, PARITY UNPINNED: the reference regrids nothing; the contract is this build's own (include/gwen_hip.h,
// "Conservative regridding"; DESIGN.md, "Conservative regridding") and is restated in numpy in tests/conserve_ref.py.
//
// A cell is V (3 .. 8) unit vectors, counter-clockwise seen from outside, joined by great-circle arcs; a cell with fewer
// corners repeats a vertex, and the zero-length edge that makes is skipped.  Everything is fp64 and the library is built
// with -ffp-contract=off, so every expression below is the one numpy evaluates:
//     dot(a, b)    (a0 b0 + a1 b1) + a2 b2
//     cross(a, b)  (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0)
//     tri(a, b, c) 2 atan2(dot(a, cross(b, c)), ((1 + dot(a, b)) + dot(b, c)) + dot(c, a))      signed solid angle
//     area(P)      (tri(P0, P1, P2) + tri(P0, P2, P3)) + ...                                    fan over vertex 0
// Overlap of source cell S and target cell T: S is clipped against the half-space dot(cross(a, b), p) >= 0 of every
// non-degenerate edge (a, b) of T in turn (Sutherland-Hodgman); the crossing of arc (p, q) is |d_p| q + |d_q| p,
// normalised.  A convex polygon gains at most one vertex per half-space, so 8 + 8 = 16 vertices hold every result; a
// vertex past the 16th is dropped, never written (it takes a non-convex input to make one).
//
// k_overlap runs ONE THREAD PER CANDIDATE PAIR -- a mesh triangle at the pole of a 0.25-degree grid has thousands of
// candidates, which one thread per target would serialise.  The two polygon buffers of a thread are indexed at run time,
// which in registers would mean scratch; they live in LDS instead, [buffer][vertex][coordinate][thread] with the thread
// fastest, so a wave's accesses to one slot are consecutive doubles whatever vertex each lane is at: 2 x 16 x 3 x 8 B =
// 768 B a thread, 48 KiB a block of 64.  No thread reads another's slice, so there is no barrier.  No atomics anywhere:
// two builds are bitwise equal.
#include "cell_list.h"

namespace {

constexpr int kMaxV = 8;                    // corners of a cell at most
constexpr int kMaxPoly = 2 * kMaxV;         // vertices of a clipped polygon at most
constexpr int kPairThreads = 64;            // one wave a block: 48 KiB of polygon buffers

struct V3 { double x, y, z; };

__device__ inline V3 load3(const double *p) { return V3{p[0], p[1], p[2]}; }
__device__ inline double dot3(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ inline V3 cross3(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ inline bool same3(V3 a, V3 b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
__device__ inline double tri(V3 a, V3 b, V3 c) {
  return 2.0 * atan2(dot3(a, cross3(b, c)), ((1.0 + dot3(a, b)) + dot3(b, c)) + dot3(c, a));
}
__device__ inline double chord2(V3 a, V3 b) {
  const double dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
  return (dx * dx + dy * dy) + dz * dz;
}

// one thread per cell: centre = the vertex sum over its length, radius = the largest chord centre -> vertex, area
__global__ __launch_bounds__(kThreads) void k_cell_areas(const double *__restrict__ cells, int64_t n, int v,
                                                         double *__restrict__ centre, double *__restrict__ radius,
                                                         double *__restrict__ area) {
  const int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (i >= n) return;
  const double *c = cells + i * (int64_t)v * 3;
  const V3 p0 = load3(c);
  V3 s = p0;
  for (int k = 1; k < v; ++k) {
    const V3 p = load3(c + 3 * k);
    s.x += p.x; s.y += p.y; s.z += p.z;
  }
  const double len = sqrt(dot3(s, s));
  const V3 m{s.x / len, s.y / len, s.z / len};
  double r2 = 0.0, a = 0.0;
  V3 prev = p0;
  for (int k = 0; k < v; ++k) {
    const V3 p = load3(c + 3 * k);
    r2 = fmax(r2, chord2(p, m));
    if (k >= 2) a += tri(p0, prev, p);
    prev = p;
  }
  centre[3 * i] = m.x; centre[3 * i + 1] = m.y; centre[3 * i + 2] = m.z;
  radius[i] = sqrt(r2);
  area[i] = a;
}

struct Poly {                               // one thread's slice of the block's polygon buffers
  double *base;                             // &lds[0][0][0][thread]
  __device__ inline V3 get(int buf, int i) const {
    const double *p = base + ((buf * kMaxPoly + i) * 3) * kPairThreads;
    return V3{p[0], p[kPairThreads], p[2 * kPairThreads]};
  }
  __device__ inline void put(int buf, int i, V3 v) const {
    double *p = base + ((buf * kMaxPoly + i) * 3) * kPairThreads;
    p[0] = v.x; p[kPairThreads] = v.y; p[2 * kPairThreads] = v.z;
  }
};

__global__ __launch_bounds__(kPairThreads) void k_overlap(const double *__restrict__ src, int vs,
                                                          const double *__restrict__ dst, int vt,
                                                          const int64_t *__restrict__ pairs, int64_t e, int64_t ns,
                                                          int64_t nd, const double *__restrict__ sc,
                                                          const double *__restrict__ sr, const double *__restrict__ dc,
                                                          const double *__restrict__ dr, double *__restrict__ out) {
  __shared__ double lds[2 * kMaxPoly * 3 * kPairThreads];
  const int64_t i = blockIdx.x * (int64_t)kPairThreads + threadIdx.x;
  if (i >= e) return;
  const int64_t s = pairs[i], t = pairs[e + i];
  if (s < 0 || s >= ns || t < 0 || t >= nd) { out[i] = 0.0; return; }          // never out of range
  const double reach = sr[s] + dr[t];
  if (chord2(load3(dc + 3 * t), load3(sc + 3 * s)) > reach * reach) { out[i] = 0.0; return; }
  const Poly P{lds + threadIdx.x};
  const double *S = src + s * (int64_t)vs * 3, *T = dst + t * (int64_t)vt * 3;
  int m = vs, cur = 0;
  for (int k = 0; k < vs; ++k) P.put(0, k, load3(S + 3 * k));
  for (int j = 0; j < vt && m > 0; ++j) {
    const V3 a = load3(T + 3 * j), b = load3(T + 3 * (j + 1 == vt ? 0 : j + 1));
    if (same3(a, b)) continue;                                                 // a zero-length edge clips nothing
    const V3 nrm = cross3(a, b);
    const int nxt = cur ^ 1;
    int o = 0;
    V3 p = P.get(cur, 0);
    double dp = dot3(nrm, p);
    for (int k = 0; k < m; ++k) {
      const V3 q = P.get(cur, k + 1 == m ? 0 : k + 1);
      const double dq = dot3(nrm, q);
      const bool in_p = dp >= 0.0, in_q = dq >= 0.0;
      if (in_p) {
        if (o < kMaxPoly) P.put(nxt, o, p);
        ++o;
      }
      if (in_p != in_q) {
        const double wp = fabs(dp), wq = fabs(dq);
        const V3 w{wp * q.x + wq * p.x, wp * q.y + wq * p.y, wp * q.z + wq * p.z};
        const double len = sqrt(dot3(w, w));
        if (o < kMaxPoly) P.put(nxt, o, V3{w.x / len, w.y / len, w.z / len});
        ++o;
      }
      p = q; dp = dq;
    }
    m = o < kMaxPoly ? o : kMaxPoly;
    cur = nxt;
  }
  double area = 0.0;
  if (m >= 3) {
    const V3 p0 = P.get(cur, 0);
    V3 prev = P.get(cur, 1);
    for (int k = 2; k < m; ++k) {
      const V3 p = P.get(cur, k);
      area += tri(p0, prev, p);
      prev = p;
    }
  }
  out[i] = area;
}

// one thread per target: its row summed in stored order in fp64, then the weights rounded once to fp32
__global__ __launch_bounds__(kThreads) void k_overlap_weights(const int64_t *__restrict__ rowptr,
                                                              const double *__restrict__ area,
                                                              const double *__restrict__ dst_area, int64_t nd, int64_t e,
                                                              int mode, float *__restrict__ w,
                                                              double *__restrict__ coverage) {
  const int64_t t = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (t >= nd) return;
  int64_t k0 = rowptr[t], k1 = rowptr[t + 1];
  k0 = k0 < 0 ? 0 : (k0 > e ? e : k0);                                         // never out of range
  k1 = k1 < k0 ? k0 : (k1 > e ? e : k1);
  double sum = 0.0;
  for (int64_t k = k0; k < k1; ++k) sum += area[k];
  const double at = dst_area[t];
  coverage[t] = sum / at;
  const double den = mode == GWEN_CONSERVE_COVERED ? sum : at;
  for (int64_t k = k0; k < k1; ++k) w[k] = (float)(area[k] / den);
}

inline bool v_ok(int v) { return v >= 3 && v <= kMaxV; }

}  // namespace

extern "C" int gwen_cell_areas(const double *cells, int64_t n, int v, double *centre, double *radius, double *area,
                               gwen_stream_t stream) {
  if (n < 0 || !v_ok(v)) return GWEN_EINVAL;
  if (n >= kIndexLimit) return GWEN_ERANGE;
  if (n == 0) return GWEN_OK;
  if (!cells || !centre || !radius || !area) return GWEN_EINVAL;
  k_cell_areas<<<blocks_for(n), kThreads, 0, gwen_stream(stream)>>>(cells, n, v, centre, radius, area);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

extern "C" int gwen_cell_overlap_areas(const double *src_cells, int64_t num_src, int vs, const double *dst_cells,
                                       int64_t num_dst, int vt, const int64_t *pairs, int64_t e,
                                       const double *src_centre, const double *src_radius, const double *dst_centre,
                                       const double *dst_radius, double *area, gwen_stream_t stream) {
  if (num_src < 0 || num_dst < 0 || e < 0 || !v_ok(vs) || !v_ok(vt)) return GWEN_EINVAL;
  if (num_src >= kIndexLimit || num_dst >= kIndexLimit || e >= kIndexLimit) return GWEN_ERANGE;
  if (e == 0) return GWEN_OK;
  if (!src_cells || !dst_cells || !pairs || !src_centre || !src_radius || !dst_centre || !dst_radius || !area)
    return GWEN_EINVAL;
  const unsigned blocks = (unsigned)((e + kPairThreads - 1) / kPairThreads);
  k_overlap<<<blocks, kPairThreads, 0, gwen_stream(stream)>>>(src_cells, vs, dst_cells, vt, pairs, e, num_src, num_dst,
                                                             src_centre, src_radius, dst_centre, dst_radius, area);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

extern "C" int gwen_cell_overlap_weights(const int64_t *rowptr, const double *area, const double *dst_area,
                                         int64_t num_dst, int64_t e, int mode, float *weights, double *coverage,
                                         gwen_stream_t stream) {
  if (num_dst < 0 || e < 0 || (mode != GWEN_CONSERVE_COVERED && mode != GWEN_CONSERVE_CELL)) return GWEN_EINVAL;
  if (num_dst >= kIndexLimit || e >= kIndexLimit) return GWEN_ERANGE;
  if (num_dst == 0) return GWEN_OK;
  if (!rowptr || !dst_area || !coverage || (e > 0 && (!area || !weights))) return GWEN_EINVAL;
  k_overlap_weights<<<blocks_for(num_dst), kThreads, 0, gwen_stream(stream)>>>(rowptr, area, dst_area, num_dst, e, mode,
                                                                              weights, coverage);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}
