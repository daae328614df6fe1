// Real spherical harmonic transforms on a latitude-longitude grid (gwen_amd.spectral), in two stages with an fp64
// intermediate ring[chunk, nlat, 2 lmax + 1, C]: column lmax + m holds the cos sum of order m over a latitude ring, column
// lmax - m the sin sum.
//
//   analysis   k_sht_lon_fwd  ring[j, m] = sum_i x[j, i] (cos, sin)(2 pi m i / nlon)          (direct sums, table twiddles)
//              k_sht_lat_fwd  c[l, +-m]  = sum_j w_j Pbar_l^m(sin lat_j) ring[j, +-m]
//   synthesis  k_sht_lat_inv  ring[j, +-m] = sum_{l >= m} c[l, +-m] Pbar_l^m(sin lat_j)
//              k_sht_lon_inv  x[j, i] = w_j sum_m ring[j, +m] cos + ring[j, -m] sin
//
// The latitude weight vector is an argument (NULL = ones), so the adjoints are the same kernels: A^T g = q * synthesis(g),
// S^T h = analysis with unit weights.  Pbar_l^m is never stored: a block owns one order m, seeds Pbar_m^m = seed[m] cos^m
// and walks the three-term recurrence in l, 32 degrees x 64 latitudes at a time through an LDS tile that its 256 threads
// contract against a tile of the ring sums (or of the coefficients).  Every sum is one thread's fp64 fma chain in index
// order (i, j, l or m ascending) over one item and one channel: no atomics, nothing depends on the batch or on how it is
// chunked, and a NaN stays in its (item, channel).
//
// With longitude = GWEN_SHT_LON_FFT (gwen_sht_transform) the two longitude kernels are k_sht_lon_fft_fwd and
// k_sht_lon_fft_inv of sht_fft.h, one fp64 FFT a ring and channel in LDS: the same ring, the same numbers up to rounding.
// lon_fwd() and lon_inv() below are the one place where the launchers choose.
//
// On a reduced Gaussian grid (gwen_sht_rings_transform: a ring length of its own on every latitude) they are
// k_sht_rings_lon_fwd and k_sht_rings_lon_inv ("reduced grids" below): the direct sums of the regular grid -- lon_sums()
// and lon_synthesis(), the one copy of either loop -- one ring a block; or, on request (gwen_sht_rings_fft_transform),
// k_sht_rings_lon_fft_fwd and k_sht_rings_lon_fft_inv of sht_fft.h, one FFT a ring, item and channel whatever the ring's
// length.
//
// The vector transforms, (u, v) <-> (vort, div), run the same longitude kernels on u and on v (ring [2, chunk, ...]) and
// the latitude kernels k_vsht_lat_fwd and k_vsht_lat_inv, with two Legendre tables and four columns where the scalar
// ones have one and two ("the latitude stage" below).  The two inverse kernels are one body, lat_inv<V>.  The two forward
// kernels call the same block decode, seed, coefficient staging and tile index and keep a body each: as one templated
// body k_vsht_lat_fwd measured 2 - 4 % slower (DESIGN, "Spherical harmonics", the refactor's A/B).
#include "common.h"
#include "sht_fft.h"

namespace {

constexpr int kThreads = 256;
constexpr int kCT = 16;          // channels of a block
constexpr int kLT = 32;          // degrees of a Legendre tile
constexpr int kJT = 64;          // latitudes of a Legendre tile
constexpr int kLonK = 16;        // orders (k_sht_lon_fwd) or longitudes (k_sht_lon_inv) of a wave, 64 a block
constexpr int kLMax = 1023;      // the plain fp64 recurrence is orthonormal to 1e-11 up to here
constexpr int kMaxLat = 2048;    // k_sht_lat_fwd keeps two recurrence values per latitude in LDS

struct dpair {
  double x, y;
};

// c^m by squaring: the sectoral seed's latitude factor
__device__ __forceinline__ double powi(double c, int m) {
  double r = 1.0;
  while (m > 0) {
    if (m & 1) r = r * c;
    c = c * c;
    m >>= 1;
  }
  return r;
}

// ---- the longitude stage: direct sums ---------------------------------------------------------------------------------
// A lane owns one (ring, channel) row of x and a wave 16 orders m (forward) or 16 longitudes i (inverse): their table
// steps, the table indices (m i) mod nlon and the twiddles are wave-uniform (scalar registers, scalar loads), and the
// vector unit issues little but the 32 fma of a longitude (order).  The two loops below are what the regular and the
// reduced grid share, so rings of one length give the bits of the regular grid; who shares a wave is the kernels' own.

// (ac, as)[k] = sum_i xp[i C] (cos, sin)(2 pi step[k] i / nlon), i ascending; tw is the ring's table
template <typename TIn>
__device__ __forceinline__ void lon_sums(const TIn *xp, const dpair *tw, int nlon, int C, const int (&step)[kLonK],
                                         double (&ac)[kLonK], double (&as)[kLonK]) {
  int idx[kLonK];
#pragma unroll
  for (int k = 0; k < kLonK; ++k) {
    idx[k] = 0;
    ac[k] = 0.0;
    as[k] = 0.0;
  }
#pragma unroll 2
  for (int i = 0; i < nlon; ++i) {
    const double xv = (double)xp[(int64_t)i * C];
#pragma unroll
    for (int k = 0; k < kLonK; ++k) {
      const dpair t = tw[idx[k]];
      ac[k] = fma(xv, t.x, ac[k]);
      as[k] = fma(xv, t.y, as[k]);
      idx[k] += step[k];
      if (idx[k] >= nlon) idx[k] -= nlon;
    }
  }
}

// acc[k] = sum_{m <= M} gp[m C] cos(2 pi m step[k] / nlon) + gp[-m C] sin(...), m ascending; gp is column 0 of a ring row
__device__ __forceinline__ void lon_synthesis(const double *gp, const dpair *tw, int nlon, int M, int C,
                                              const int (&step)[kLonK], double (&acc)[kLonK]) {
  int idx[kLonK];
#pragma unroll
  for (int k = 0; k < kLonK; ++k) {
    idx[k] = 0;
    acc[k] = 0.0;
  }
#pragma unroll 2
  for (int m = 0; m <= M; ++m) {
    const double gc = gp[(int64_t)m * C];
    const double gs = m ? gp[-(int64_t)m * C] : 0.0;
#pragma unroll
    for (int k = 0; k < kLonK; ++k) {
      const dpair w = tw[idx[k]];
      acc[k] = fma(gc, w.x, acc[k]);
      acc[k] = fma(gs, w.y, acc[k]);
      idx[k] += step[k];
      if (idx[k] >= nlon) idx[k] -= nlon;
    }
  }
}

// Rows run over (item, latitude, channel), so every lane works whatever C is.
template <typename TIn>
__global__ __launch_bounds__(kThreads) void k_sht_lon_fwd(const TIn *__restrict__ x, const dpair *__restrict__ tw,
                                                          double *__restrict__ ring, int64_t rows, int nlon, int L, int C,
                                                          int mtiles) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int mt = (int)(blockIdx.x % mtiles);
  const int64_t r = (int64_t)(blockIdx.x / mtiles) * 64 + lane;
  const int64_t rr = r < rows ? r : rows - 1;              // a lane past the end reads the last row and stores nothing
  const int64_t row = rr / C;                              // item * nlat + j
  const int c = (int)(rr - row * C);
  const int m0 = __builtin_amdgcn_readfirstlane((mt * 4 + wave) * kLonK);
  if (m0 > L) return;
  int mk[kLonK];
  double ac[kLonK], as[kLonK];
#pragma unroll
  for (int k = 0; k < kLonK; ++k) mk[k] = m0 + k <= L ? m0 + k : 0;   // past lmax: walks order 0, is not stored
  lon_sums(x + row * (int64_t)nlon * C + c, tw, nlon, C, mk, ac, as);
  if (r >= rows) return;
  double *out = ring + (row * (int64_t)(2 * L + 1) + L) * C + c;
#pragma unroll
  for (int k = 0; k < kLonK; ++k) {
    const int m = m0 + k;
    if (m > L) continue;
    out[(int64_t)m * C] = ac[k];
    if (m > 0) out[-(int64_t)m * C] = as[k];
  }
}

template <typename TOut>
__global__ __launch_bounds__(kThreads) void k_sht_lon_inv(const double *__restrict__ ring, const dpair *__restrict__ tw,
                                                          const double *__restrict__ lat_w, TOut *__restrict__ x,
                                                          int64_t rows, int nlat, int nlon, int L, int C, int itiles) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int it = (int)(blockIdx.x % itiles);
  const int64_t r = (int64_t)(blockIdx.x / itiles) * 64 + lane;
  const int64_t rr = r < rows ? r : rows - 1;
  const int64_t row = rr / C;                              // item * nlat + j
  const int c = (int)(rr - row * C);
  const int i0 = __builtin_amdgcn_readfirstlane((it * 4 + wave) * kLonK);
  if (i0 >= nlon) return;
  int step[kLonK];
  double acc[kLonK];
#pragma unroll
  for (int k = 0; k < kLonK; ++k) step[k] = i0 + k < nlon ? i0 + k : 0;
  lon_synthesis(ring + (row * (int64_t)(2 * L + 1) + L) * C + c, tw, nlon, L, C, step, acc);
  if (r >= rows) return;
  const double w = lat_w ? lat_w[row % nlat] : 1.0;
  TOut *xo = x + row * (int64_t)nlon * C + c;
#pragma unroll
  for (int k = 0; k < kLonK; ++k)
    if (i0 + k < nlon) xo[(int64_t)(i0 + k) * C] = (TOut)(acc[k] * w);
}

// ---- reduced grids: rings of unequal length (gwen_sht_rings_transform) ----------------------------------------------
// Ring j holds ring_nlon[j] longitudes 2 pi i / ring_nlon[j], the rows ring_start[j] ... of an item's P points, and
// carries the orders m <= M_j = min(lmax, (ring_nlon[j] - 1) / 2); tw is one table a ring, end to end, tw[ring_start[j] +
// i] = (cos, sin)(2 pi i / ring_nlon[j]).  The sums are lon_sums() and lon_synthesis().  What changes is who shares a
// wave: a block owns one ring, 64 (item, channel) lanes and 64 orders (longitudes), so the ring's length, start and M_j
// are block-uniform and the table indices and twiddles stay in scalar registers.  The forward kernel stores zeros in the
// columns of the orders above M_j (the latitude kernels read every column, and the workspace arrives uninitialised); the
// inverse kernel does not read them.

// Rows of blocks take the rings from the equator outwards (ring_of(), sht_fft.h).
using sht_fft::ring_of;

template <typename TIn>
__global__ __launch_bounds__(kThreads) void k_sht_rings_lon_fwd(const TIn *__restrict__ x, const dpair *__restrict__ tw,
                                                                const int *__restrict__ ring_nlon,
                                                                const int64_t *__restrict__ ring_start,
                                                                double *__restrict__ ring, int64_t lanes, int64_t P,
                                                                int nlat, int L, int C, int mtiles, int ltiles) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int blk = (int)blockIdx.x;
  const int mt = blk % mtiles;
  blk /= mtiles;
  const int lt = blk % ltiles;
  const int j = ring_of(blk / ltiles, nlat);
  const int nlon = ring_nlon[j];
  const int M = L < ((nlon - 1) >> 1) ? L : (nlon - 1) >> 1;
  const int m0 = __builtin_amdgcn_readfirstlane((mt * 4 + wave) * kLonK);
  if (m0 > L) return;
  const int64_t q = (int64_t)lt * 64 + lane;
  const int64_t qq = q < lanes ? q : lanes - 1;           // a lane past the end reads the last one and stores nothing
  const int64_t item = qq / C;
  const int c = (int)(qq - item * C);
  double *out = ring + ((item * nlat + j) * (int64_t)(2 * L + 1) + L) * C + c;
  if (m0 > M) {                                           // a wave of truncated orders (all of them >= 1): zeros, and done
    if (q >= lanes) return;
#pragma unroll
    for (int k = 0; k < kLonK; ++k) {
      const int m = m0 + k;
      if (m > L) continue;
      out[(int64_t)m * C] = 0.0;
      out[-(int64_t)m * C] = 0.0;
    }
    return;
  }
  int mk[kLonK];
  double ac[kLonK], as[kLonK];
#pragma unroll
  for (int k = 0; k < kLonK; ++k) mk[k] = m0 + k <= M ? m0 + k : 0;   // past M_j: walks order 0, is stored as zero
  const int64_t start = ring_start[j];
  lon_sums(x + (item * P + start) * C + c, tw + start, nlon, C, mk, ac, as);
  if (q >= lanes) return;
#pragma unroll
  for (int k = 0; k < kLonK; ++k) {
    const int m = m0 + k;
    if (m > L) continue;
    out[(int64_t)m * C] = m <= M ? ac[k] : 0.0;
    if (m > 0) out[-(int64_t)m * C] = m <= M ? as[k] : 0.0;
  }
}

template <typename TOut>
__global__ __launch_bounds__(kThreads) void k_sht_rings_lon_inv(const double *__restrict__ ring,
                                                                const dpair *__restrict__ tw,
                                                                const int *__restrict__ ring_nlon,
                                                                const int64_t *__restrict__ ring_start,
                                                                const double *__restrict__ lat_w, TOut *__restrict__ x,
                                                                int64_t lanes, int64_t P, int nlat, int L, int C,
                                                                int itiles, int ltiles) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int blk = (int)blockIdx.x;
  const int it = blk % itiles;
  blk /= itiles;
  const int lt = blk % ltiles;
  const int j = ring_of(blk / ltiles, nlat);
  const int nlon = ring_nlon[j];
  const int M = L < ((nlon - 1) >> 1) ? L : (nlon - 1) >> 1;
  const int i0 = __builtin_amdgcn_readfirstlane((it * 4 + wave) * kLonK);
  if (i0 >= nlon) return;
  const int64_t q = (int64_t)lt * 64 + lane;
  const int64_t qq = q < lanes ? q : lanes - 1;
  const int64_t item = qq / C;
  const int c = (int)(qq - item * C);
  int step[kLonK];
  double acc[kLonK];
#pragma unroll
  for (int k = 0; k < kLonK; ++k) step[k] = i0 + k < nlon ? i0 + k : 0;
  const int64_t start = ring_start[j];
  lon_synthesis(ring + ((item * nlat + j) * (int64_t)(2 * L + 1) + L) * C + c, tw + start, nlon, M, C, step, acc);
  if (q >= lanes) return;
  const double w = lat_w ? lat_w[j] : 1.0;
  TOut *xo = x + (item * P + start) * C + c;
#pragma unroll
  for (int k = 0; k < kLonK; ++k)
    if (i0 + k < nlon) xo[(int64_t)(i0 + k) * C] = (TOut)(acc[k] * w);
}

// S_l = sum_m c_lm^2, m = -l ... l in that order; one thread per (item, l, channel)
__global__ __launch_bounds__(kThreads) void k_sht_power(const double *__restrict__ coef, double *__restrict__ power,
                                                        int64_t total, int L, int C) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % C);
  const int64_t r = e / C;
  const int l = (int)(r % (L + 1));
  const int64_t item = r / (L + 1);
  const double *p = coef + (item * (int64_t)(L + 1) * (L + 1) + (int64_t)l * l) * C + c;
  double s = 0.0;
  for (int k = 0; k <= 2 * l; ++k) {
    const double v = p[(int64_t)k * C];
    s = fma(v, v, s);
  }
  power[e] = s;
}

// ---- the latitude stage, scalar (V = false) or vector (V = true) -----------------------------------------------------
// Scalar: the table is Pbar_l^m, the columns are the cos and the sin sums (coefficients) of order m.
//
// Vector, (u, v) <-> (vort, div): grad Y of the cos row (l, m >= 0) is (east, north) = (-m Q sin m lon, D cos m lon), of
// the sin row (l, -m) it is (m Q cos m lon, D sin m lon), with Q = Pbar_l^m / cos lat and D = d Pbar_l^m / d lat; k x grad
// Y = (-north, east).  Neither table divides by cos lat.  For m >= 1 the block walks Q_l^m, the recurrence of Pbar_l^m
// seeded one cosine short (seed[m] cos^(m-1) lat), and D_l^m = c_d Q_{l-1}^m - l sin lat Q_l^m.  For m = 0 the Q term
// carries the factor m = 0 and D_l^0 = c_d Pbar_l^1, so the block walks the order-1 recurrence from l = 1.  Either way one
// recurrence a latitude, two tables (m Q, D) and four columns: (u cos, u sin, v cos, v sin) or those of (vort, div).

// a, b of Pbar_l^m = a (mu Pbar_{l-1}^m - b Pbar_{l-2}^m), l > m (l = m + 1: a = sqrt(2m + 3), b = 0)
__device__ __forceinline__ void recurrence_coefficients(int l, int m, double &a, double &b) {
  const double dl = (double)l, dm = (double)m, dl1 = (double)(l - 1);
  a = sqrt((4.0 * dl * dl - 1.0) / (dl * dl - dm * dm));
  b = sqrt((dl1 * dl1 - dm * dm) / (4.0 * dl1 * dl1 - 1.0));
}

// c_d of D above: sqrt((2l + 1)(l^2 - m^2) / (2l - 1)) for m >= 1, sqrt(l (l + 1) / 2) for m = 0
__device__ __forceinline__ double derivative_coefficient(int l, int m) {
  const double dl = (double)l, dm = (double)m;
  return m ? sqrt((2.0 * dl + 1.0) * (dl * dl - dm * dm) / (2.0 * dl - 1.0)) : sqrt(dl * (dl + 1.0) / 2.0);
}

// the order of the recurrence that a block of order m walks
template <bool V>
__device__ __forceinline__ int walk_order(int m) {
  return V && m == 0 ? 1 : m;
}

// The walk's first value at a latitude of cosine cl.  lmax = 0, vector: seed has one entry, and nothing reads the walk.
template <bool V>
__device__ __forceinline__ double walk_seed(const double *__restrict__ seed, int m, int L, double cl) {
  const int mm = walk_order<V>(m);
  return seed[mm < L ? mm : L] * powi(cl, V ? (m ? m - 1 : 1) : m);
}

// The recurrence coefficients of the nl degrees from l0 on, one degree a thread: co [2 + V][kLT] holds a, b and, when V,
// c_d.  The scalar kernels have no third row.
template <bool V>
__device__ __forceinline__ void stage_coefficients(double *co, int l0, int nl, int m) {
  const int t = threadIdx.x, mm = walk_order<V>(m);
  if (t >= nl) return;
  double a = 0.0, b = 0.0;
  if (l0 + t > mm) recurrence_coefficients(l0 + t, mm, a, b);
  co[t] = a;
  co[kLT + t] = b;
  if constexpr (V) co[2 * kLT + t] = derivative_coefficient(l0 + t, m);
}

// One degree l of the walk, scalar: p1 = Pbar_l^m (p2 = Pbar_{l-1}^m) on the way out; c points at the staged a of l, b is
// kLT further on.
__device__ __forceinline__ void scalar_step(int l, int m, double mu, const double *c, double &p1, double &p2, double &p) {
  if (l > m) {
    const double n = c[0] * (mu * p1 - c[kLT] * p2);
    p2 = p1;
    p1 = n;
  }
  p = p1;
}

// One degree l of the walk, vector: p1 = the recurrence value of degree l (p2 of l - 1) on the way out, (q, d) =
// (m Q_l^m, D_l^m); a, b and cd are the staged coefficients of l.  The walk is one wave's serial chain while the block's
// other three wait, and how it reads the coefficients shows in the time: the kernels read these three by value ahead of
// the call (a select a degree), the scalar step reads its two where it needs them.  Measure before merging the two.
__device__ __forceinline__ void vector_step(int l, int m, double mu, double a, double b, double cd, double &p1,
                                            double &p2, double &q, double &d) {
  if (l > walk_order<true>(m)) {
    const double p = a * (mu * p1 - b * p2);
    p2 = p1;
    p1 = p;
  }
  if (m) {
    q = (double)m * p1;
    d = cd * p2 - (double)l * mu * p1;
  } else {
    q = 0.0;
    d = l ? cd * p1 : 0.0;
  }
}

// Degree t, latitude j of a Legendre tile [kLT][kJT]: column (j + t) & 63, conflict-free for the writer's 64 latitudes
// and for the readers' 4 degrees a wave.
__device__ __forceinline__ int tile_at(int t, int j) { return t * kJT + ((j + t) & (kJT - 1)); }

// One table entry against one latitude's (degree's) columns.  Scalar, either direction: (cos, sin) += Pbar (cos, sin).
__device__ __forceinline__ void contract(const double (&p)[1], const double (&f)[2], double (&acc)[2]) {
  acc[0] = fma(p[0], f[0], acc[0]);
  acc[1] = fma(p[0], f[1], acc[1]);
}

// Vector synthesis: f = (psi cos, psi sin, chi cos, chi sin), acc = (u cos, u sin, v cos, v sin), (u, v) = sum psi k x
// grad Y + chi grad Y.  (The vector analysis has its four lines in k_vsht_lat_fwd.)
__device__ __forceinline__ void contract(const double (&p)[2], const double (&f)[4], double (&acc)[4]) {
  const double q = p[0], d = p[1];
  acc[0] = fma(q, f[3], fma(-d, f[0], acc[0]));        // u, cos column: -D psi_cos + m Q chi_sin
  acc[1] = fma(-q, f[2], fma(-d, f[1], acc[1]));       // u, sin column: -D psi_sin - m Q chi_cos
  acc[2] = fma(d, f[2], fma(q, f[1], acc[2]));         // v, cos column:  m Q psi_sin + D chi_cos
  acc[3] = fma(d, f[3], fma(-q, f[0], acc[3]));        // v, sin column: -m Q psi_cos + D chi_sin
}

// What the inverse kernels make of a coefficient of degree l: the scalar one takes it as it is; the vector one reads a
// NULL tensor and row 0 as 0 and takes the potentials psi = -vort / L and chi = -div / L (unit_L = 0) or -vort, -div
// (unit_L = 1, the adjoint of the analysis, whose factor L cancels).
template <bool V, typename TIn>
__device__ __forceinline__ double loaded_coefficient(const TIn *tensor, int64_t at, int l, int unit_L) {
  if constexpr (!V) return (double)tensor[at];
  if (!tensor || l == 0) return 0.0;
  const double raw = (double)tensor[at];
  return unit_L ? -raw : -raw / ((double)l * (double)(l + 1));
}

// Blocks run over (item, channel tile, order m, latitude tile), the last the fastest; the forward kernels have one
// latitude tile.
struct LatBlock {
  int jt, m, ct;
  int64_t item;
};
__device__ __forceinline__ LatBlock lat_block(int L, int ctiles, int jtiles) {
  LatBlock b;
  int64_t blk = blockIdx.x;
  b.jt = (int)(blk % jtiles);
  blk /= jtiles;
  b.m = (int)(blk % (L + 1));
  blk /= (L + 1);
  b.ct = (int)(blk % ctiles);
  b.item = blk / ctiles;
  return b;
}

// Forward, scalar.  Block (item, channel tile, order m): all latitudes, all degrees l >= m.  Dynamic LDS (lat_fwd_lds):
// two recurrence values per latitude, the Legendre tile with the latitude weight in it, the ring tile and the recurrence
// coefficients of the tile's degrees.  Thread (channel, 2 degrees) sums over the latitudes.
template <typename TOut>
__global__ __launch_bounds__(kThreads) void k_sht_lat_fwd(const double *__restrict__ ring, const dpair *__restrict__ nodes,
                                                          const double *__restrict__ lat_w,
                                                          const double *__restrict__ seed, TOut *__restrict__ coef,
                                                          int nlat, int L, int C, int ctiles) {
  extern __shared__ double smem[];
  double *st1 = smem;                                     // [nlat]  Pbar_{l-1}^m at the start of a degree tile
  double *st2 = st1 + nlat;                               // [nlat]  Pbar_{l-2}^m
  double *pt = st2 + nlat;                                // [kLT][kJT]  Pbar w
  double *ft = pt + kLT * kJT;                            // [kJT][2][kCT]
  double *co = ft + kJT * 2 * kCT;                        // [2][kLT]
  const int tid = threadIdx.x, cl = tid & (kCT - 1), lg = tid >> 4;
  const LatBlock b = lat_block(L, ctiles, 1);
  const int m = b.m, c = b.ct * kCT + cl;
  const int64_t T = (int64_t)(L + 1) * (L + 1);
  for (int j = tid; j < nlat; j += kThreads) {
    st1[j] = walk_seed<false>(seed, m, L, nodes[j].y);
    st2[j] = 0.0;
  }
  const double *fr = ring + b.item * (int64_t)nlat * (2 * L + 1) * C;
  for (int l0 = m; l0 <= L; l0 += kLT) {
    const int nl = L - l0 + 1 < kLT ? L - l0 + 1 : kLT;
    __syncthreads();                                      // the tile before is done with co (and st1, st2 are set)
    stage_coefficients<false>(co, l0, nl, m);
    double acc[2][2] = {};
    for (int j0 = 0; j0 < nlat; j0 += kJT) {
      __syncthreads();
      if (tid < kJT) {
        const int j = j0 + tid;
        if (j < nlat) {
          double p1 = st1[j], p2 = st2[j];
          const double mu = nodes[j].x, w = lat_w ? lat_w[j] : 1.0;
          for (int t = 0; t < nl; ++t) {
            double p;
            scalar_step(l0 + t, m, mu, co + t, p1, p2, p);
            pt[tile_at(t, tid)] = p * w;
          }
          st1[j] = p1;
          st2[j] = p2;
        } else {
          for (int t = 0; t < nl; ++t) pt[tile_at(t, tid)] = 0.0;
        }
      }
#pragma unroll
      for (int r = 0; r < kJT * 2 * kCT / kThreads; ++r) {
        const int e = tid + kThreads * r, cc = e & (kCT - 1), kk = (e >> 4) & 1, jj = e >> 5;
        const int j = j0 + jj, gc = b.ct * kCT + cc;
        ft[e] = j < nlat && gc < C ? fr[((int64_t)j * (2 * L + 1) + (kk ? L - m : L + m)) * C + gc] : 0.0;
      }
      __syncthreads();
      const int nj = nlat - j0 < kJT ? nlat - j0 : kJT;
      for (int jj = 0; jj < nj; ++jj) {
        const double f[2] = {ft[(jj * 2 + 0) * kCT + cl], ft[(jj * 2 + 1) * kCT + cl]};
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int t = lg + 16 * r;
          const double p[1] = {t < nl ? pt[tile_at(t, jj)] : 0.0};
          contract(p, f, acc[r]);
        }
      }
    }
    if (c < C) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int l = l0 + lg + 16 * r;
        if (l > L) continue;
        TOut *o = coef + (b.item * T + (int64_t)l * l + l) * C + c;
        o[(int64_t)m * C] = (TOut)acc[r][0];
        if (m > 0) o[-(int64_t)m * C] = (TOut)acc[r][1];
      }
    }
  }
}

// Block (item, channel tile, order m) as k_sht_lat_fwd, with two tables (m Q w, D w) and four ring columns (u cos, u sin,
// v cos, v sin) in LDS.  vort_lm = sum_j w (u, v) . (D, m Q) {cos, sin}-wise and div_lm likewise (signs below), stored
// as they are (inv_L = 0) or over L = l (l + 1) (inv_L = 1, the adjoint of the synthesis); row 0 is stored as 0.
template <typename TOut>
__global__ __launch_bounds__(kThreads) void k_vsht_lat_fwd(const double *__restrict__ ring_u,
                                                           const double *__restrict__ ring_v,
                                                           const dpair *__restrict__ nodes,
                                                           const double *__restrict__ lat_w,
                                                           const double *__restrict__ seed, TOut *__restrict__ vort,
                                                           TOut *__restrict__ div, int nlat, int L, int C, int ctiles,
                                                           int inv_L) {
  extern __shared__ double smem[];
  double *st1 = smem;                                     // [nlat]  the recurrence at l - 1, at the start of a degree tile
  double *st2 = st1 + nlat;                               // [nlat]  at l - 2
  double *qt = st2 + nlat;                                // [kLT][kJT]  m Q w
  double *dt = qt + kLT * kJT;                            // [kLT][kJT]  D w
  double *ft = dt + kLT * kJT;                            // [kJT][4][kCT]
  double *ca = ft + kJT * 4 * kCT;                        // [3][kLT]: a, b, c_d (stage_coefficients)
  double *cb = ca + kLT;
  double *cd = cb + kLT;
  const int tid = threadIdx.x, cl = tid & (kCT - 1), lg = tid >> 4;
  const LatBlock b = lat_block(L, ctiles, 1);
  const int m = b.m, c = b.ct * kCT + cl;
  const int64_t T = (int64_t)(L + 1) * (L + 1);
  for (int j = tid; j < nlat; j += kThreads) {
    st1[j] = walk_seed<true>(seed, m, L, nodes[j].y);
    st2[j] = 0.0;
  }
  const int64_t item_off = b.item * (int64_t)nlat * (2 * L + 1) * C;
  for (int l0 = m; l0 <= L; l0 += kLT) {
    const int nl = L - l0 + 1 < kLT ? L - l0 + 1 : kLT;
    __syncthreads();                                      // the tile before is done with ca, cb, cd
    stage_coefficients<true>(ca, l0, nl, m);
    double acc[2][4] = {};
    for (int j0 = 0; j0 < nlat; j0 += kJT) {
      __syncthreads();
      if (tid < kJT) {
        const int j = j0 + tid;
        if (j < nlat) {
          double p1 = st1[j], p2 = st2[j];
          const double mu = nodes[j].x, w = lat_w ? lat_w[j] : 1.0;
          for (int t = 0; t < nl; ++t) {
            double q, d;
            vector_step(l0 + t, m, mu, ca[t], cb[t], cd[t], p1, p2, q, d);
            qt[tile_at(t, tid)] = q * w;
            dt[tile_at(t, tid)] = d * w;
          }
          st1[j] = p1;
          st2[j] = p2;
        } else {
          for (int t = 0; t < nl; ++t) {
            qt[tile_at(t, tid)] = 0.0;
            dt[tile_at(t, tid)] = 0.0;
          }
        }
      }
#pragma unroll
      for (int r = 0; r < kJT * 4 * kCT / kThreads; ++r) {
        const int e = tid + kThreads * r, cc = e & (kCT - 1), kk = (e >> 4) & 3, jj = e >> 6;
        const int j = j0 + jj, gc = b.ct * kCT + cc;
        const double *fr = (kk & 2 ? ring_v : ring_u) + item_off;
        ft[e] = j < nlat && gc < C ? fr[((int64_t)j * (2 * L + 1) + (kk & 1 ? L - m : L + m)) * C + gc] : 0.0;
      }
      __syncthreads();
      const int nj = nlat - j0 < kJT ? nlat - j0 : kJT;
      for (int jj = 0; jj < nj; ++jj) {
        const double uc = ft[(jj * 4 + 0) * kCT + cl], us = ft[(jj * 4 + 1) * kCT + cl];
        const double vc = ft[(jj * 4 + 2) * kCT + cl], vs = ft[(jj * 4 + 3) * kCT + cl];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int t = lg + 16 * r;
          const double q = t < nl ? qt[tile_at(t, jj)] : 0.0;
          const double d = t < nl ? dt[tile_at(t, jj)] : 0.0;
          acc[r][0] = fma(q, vs, fma(d, uc, acc[r][0]));     // vort, cos row:  D u_cos + m Q v_sin
          acc[r][1] = fma(-q, vc, fma(d, us, acc[r][1]));    // vort, sin row:  D u_sin - m Q v_cos
          acc[r][2] = fma(-d, vc, fma(q, us, acc[r][2]));    // div, cos row:   m Q u_sin - D v_cos
          acc[r][3] = fma(-d, vs, fma(-q, uc, acc[r][3]));   // div, sin row:  -m Q u_cos - D v_sin
        }
      }
    }
    if (c < C) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int l = l0 + lg + 16 * r;
        if (l > L) continue;
        const double big = (double)l * (double)(l + 1);
        const int64_t o = (b.item * T + (int64_t)l * l + l) * C + c;
        double out[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = l == 0 ? 0.0 : inv_L ? acc[r][k] / big : acc[r][k];
        vort[o + (int64_t)m * C] = (TOut)out[0];
        div[o + (int64_t)m * C] = (TOut)out[2];
        if (m > 0) {
          vort[o - (int64_t)m * C] = (TOut)out[1];
          div[o - (int64_t)m * C] = (TOut)out[3];
        }
      }
    }
  }
}

// Inverse.  Block (item, channel tile, order m, 64 latitudes): the recurrence lives in the registers of the block's
// first 64 threads; thread (channel, 4 latitudes) sums over the degrees.  The sin row of order 0 reads as 0.  in1, out1:
// the vector kernel's div and v ring.
template <bool V, typename TIn>
__device__ __forceinline__ void lat_inv(const TIn *__restrict__ in0, const TIn *__restrict__ in1,
                                        const dpair *__restrict__ nodes, const double *__restrict__ seed,
                                        double *__restrict__ out0, double *__restrict__ out1, int nlat, int L, int C,
                                        int ctiles, int jtiles, int unit_L) {
  constexpr int NT = V ? 2 : 1, NC = 2 * NT;
  __shared__ double tab[NT * kLT * kJT];
  __shared__ double ctile[kLT * NC * kCT];
  __shared__ double co[(2 + V) * kLT];
  const int tid = threadIdx.x, cl = tid & (kCT - 1), jg = tid >> 4;
  const LatBlock b = lat_block(L, ctiles, jtiles);
  const int m = b.m, c = b.ct * kCT + cl;
  const int64_t T = (int64_t)(L + 1) * (L + 1);
  const int j0 = b.jt * kJT;
  const int jmine = j0 + tid;
  double p1 = 0.0, p2 = 0.0, mu = 0.0;
  if (tid < kJT && jmine < nlat) {
    p1 = walk_seed<V>(seed, m, L, nodes[jmine].y);
    mu = nodes[jmine].x;
  }
  double acc[4][NC] = {};
  for (int l0 = m; l0 <= L; l0 += kLT) {
    const int nl = L - l0 + 1 < kLT ? L - l0 + 1 : kLT;
    __syncthreads();
    stage_coefficients<V>(co, l0, nl, m);
#pragma unroll
    for (int r = 0; r < kLT * NC * kCT / kThreads; ++r) {
      const int e = tid + kThreads * r, cc = e & (kCT - 1), kk = (e >> 4) & (NC - 1), t = e / (NC * kCT);
      const int l = l0 + t, gc = b.ct * kCT + cc;
      const int64_t at = (b.item * T + (int64_t)l * l + l + (kk & 1 ? -m : m)) * C + gc;
      const bool there = l <= L && gc < C && !((kk & 1) && m == 0);
      ctile[e] = there ? loaded_coefficient<V>(kk & 2 ? in1 : in0, at, l, unit_L) : 0.0;
    }
    __syncthreads();
    if (tid < kJT) {
      for (int t = 0; t < nl; ++t) {
        double val[NT];
        if constexpr (V)
          vector_step(l0 + t, m, mu, co[t], co[kLT + t], co[2 * kLT + t], p1, p2, val[0], val[NT - 1]);
        else
          scalar_step(l0 + t, m, mu, co + t, p1, p2, val[0]);
#pragma unroll
        for (int k = 0; k < NT; ++k) tab[k * kLT * kJT + tile_at(t, tid)] = val[k];
      }
    }
    __syncthreads();
    for (int t = 0; t < nl; ++t) {
      double f[NC];
#pragma unroll
      for (int k = 0; k < NC; ++k) f[k] = ctile[(t * NC + k) * kCT + cl];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double p[NT];
#pragma unroll
        for (int k = 0; k < NT; ++k) p[k] = tab[k * kLT * kJT + tile_at(t, jg + 16 * r)];
        contract(p, f, acc[r]);
      }
    }
  }
  if (c >= C) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = j0 + jg + 16 * r;
    if (j >= nlat) continue;
    const int64_t o = ((b.item * nlat + j) * (int64_t)(2 * L + 1) + L) * C + c;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      double *out = k ? out1 : out0;
      out[o + (int64_t)m * C] = acc[r][2 * k];
      if (m > 0) out[o - (int64_t)m * C] = acc[r][2 * k + 1];
    }
  }
}

template <typename TIn>
__global__ __launch_bounds__(kThreads) void k_sht_lat_inv(const TIn *__restrict__ coef, const dpair *__restrict__ nodes,
                                                          const double *__restrict__ seed, double *__restrict__ ring,
                                                          int nlat, int L, int C, int ctiles, int jtiles) {
  lat_inv<false, TIn>(coef, nullptr, nodes, seed, ring, nullptr, nlat, L, C, ctiles, jtiles, 0);
}

template <typename TIn>
__global__ __launch_bounds__(kThreads) void k_vsht_lat_inv(const TIn *__restrict__ vort, const TIn *__restrict__ div,
                                                           const dpair *__restrict__ nodes,
                                                           const double *__restrict__ seed, double *__restrict__ ring_u,
                                                           double *__restrict__ ring_v, int nlat, int L, int C,
                                                           int ctiles, int jtiles, int unit_L) {
  lat_inv<true, TIn>(vort, div, nodes, seed, ring_u, ring_v, nlat, L, C, ctiles, jtiles, unit_L);
}

struct Shape {
  int nlat, nlon, L, C, ctiles, mtiles, itiles, jtiles;
  int64_t item_bytes, item_blocks;
  int longitude;                 // GWEN_SHT_LON_*
  sht_fft::Plan fft;             // longitude == GWEN_SHT_LON_FFT: the butterfly schedule and the channel tile
  int fft_ctiles;
  int64_t points;                // grid points of an item: nlat nlon, or the sum of the ring lengths
  const int *ring_nlon;          // a reduced grid (check_rings_shape): the device tables of the ring lengths [nlat] and
  const int64_t *ring_start;     // starts [nlat + 1]; nlon is then the longest ring.  NULL on a regular grid
  sht_fft::RingTables ring_fft;  // a reduced grid with one FFT a ring (gwen_sht_rings_fft_transform); plan NULL without
  int ring_lds_slots;            // the complex LDS slots of a block of its kernels
};

// The device tables and the point count of a reduced grid, the fields of gwen_sht_rings_call that gwen_sht_call lacks.
struct Rings {
  const int *nlon;
  const int64_t *start;
  int64_t points;
  const gwen_sht_rings_fft_call *fft;      // the call that asks for one FFT a ring, for its plan records and tables, or NULL
};

// the sizes and tile counts of checked arguments; nlon is the longest ring of a reduced grid
void set_sizes(Shape &s, int64_t nlat, int64_t nlon, int64_t lmax, int64_t C) {
  s.nlat = (int)nlat;
  s.nlon = (int)nlon;
  s.L = (int)lmax;
  s.C = (int)C;
  s.ctiles = (int)((C + kCT - 1) / kCT);
  s.mtiles = (s.L + 4 * kLonK) / (4 * kLonK);
  s.itiles = (s.nlon + 4 * kLonK - 1) / (4 * kLonK);
  s.jtiles = (s.nlat + kJT - 1) / kJT;
  s.item_bytes = nlat * (2 * lmax + 1) * C * (int64_t)sizeof(double);
}

// sizes only; 0 = fine
int check_shape(int grid, int64_t nlat, int64_t nlon, int64_t lmax, int64_t C, Shape &s,
                int longitude = GWEN_SHT_LON_DIRECT) {
  if (longitude != GWEN_SHT_LON_DIRECT && longitude != GWEN_SHT_LON_FFT) return GWEN_EINVAL;
  if (grid != GWEN_SHT_EQUIANGULAR && grid != GWEN_SHT_EQUIANGULAR_CENTRED && grid != GWEN_SHT_GAUSS) return GWEN_EINVAL;
  if (nlat < (grid == GWEN_SHT_EQUIANGULAR ? 2 : 1) || nlat > kMaxLat || nlon < 1 || C < 1) return GWEN_EINVAL;
  if (lmax < 0 || lmax > kLMax) return GWEN_EINVAL;
  if (lmax > (grid == GWEN_SHT_GAUSS ? nlat - 1 : (nlat - 1) / 2)) return GWEN_EINVAL;
  if (nlon < 2 * lmax + 1) return GWEN_EINVAL;
  if (nlat * nlon > INT32_MAX || C > INT32_MAX) return GWEN_ERANGE;      // (lmax + 1)^2 <= 2^20
  set_sizes(s, nlat, nlon, lmax, C);
  const int64_t lon = ((nlat * C + 63) / 64 + 1) * (int64_t)(s.mtiles > s.itiles ? s.mtiles : s.itiles);
  const int64_t lat = s.ctiles * (lmax + 1) * (int64_t)s.jtiles;
  s.item_blocks = lon > lat ? lon : lat;
  s.longitude = longitude;
  s.points = nlat * nlon;
  s.ring_nlon = nullptr;
  s.ring_start = nullptr;
  s.ring_fft = {};
  s.ring_lds_slots = 0;
  if (longitude == GWEN_SHT_LON_FFT) {
    if (!sht_fft::supported(nlon)) return GWEN_EINVAL;
    s.fft = sht_fft::make_plan(s.nlon, s.C);
    s.fft_ctiles = (s.C + s.fft.tile - 1) / s.fft.tile;
    // blocks (ring, channel tile), the rings rounded up to the XCD count: at most nlat + kXcds - 1 rings an item
    s.item_blocks = (nlat + sht_fft::kXcds - 1) * (int64_t)s.fft_ctiles;
    if (lat > s.item_blocks) s.item_blocks = lat;
  }
  return 0;
}

// A reduced grid: nlat Gauss latitudes, `points` grid points in rings of at most max_nlon.  Sizes only; 0 = fine.  What
// the tables hold is the caller's business.
int check_rings_shape(const Rings &r, int64_t nlat, int64_t max_nlon, int64_t lmax, int64_t C, Shape &s) {
  if (nlat < 1 || nlat > kMaxLat || max_nlon < 1 || C < 1) return GWEN_EINVAL;
  if (lmax < 0 || lmax > kLMax || lmax > nlat - 1) return GWEN_EINVAL;
  if (max_nlon < 2 * lmax + 1) return GWEN_EINVAL;
  if (r.points > INT32_MAX || max_nlon > INT32_MAX || C > INT32_MAX) return GWEN_ERANGE;
  // every ring has a point and none more than max_nlon, which one of them has
  if (r.points < nlat - 1 + max_nlon || r.points > nlat * max_nlon) return GWEN_EINVAL;
  set_sizes(s, nlat, max_nlon, lmax, C);
  // blocks (ring, 64 (item, channel) lanes, 64 orders or longitudes): at most ceil(C / 64) lane tiles an item
  const int64_t lon = nlat * ((C + 63) / 64) * (int64_t)(s.mtiles > s.itiles ? s.mtiles : s.itiles);
  const int64_t lat = s.ctiles * (lmax + 1) * (int64_t)s.jtiles;
  s.item_blocks = lon > lat ? lon : lat;
  s.longitude = GWEN_SHT_LON_DIRECT;
  s.fft_ctiles = 0;
  s.points = r.points;
  s.ring_nlon = r.nlon;
  s.ring_start = r.start;
  s.ring_fft = {};
  s.ring_lds_slots = 0;
  if (r.fft) {
    // blocks (ring, item, channel tile) with the tile of the ring that has the most points in LDS, the rows rounded up to
    // the XCD count
    const int64_t most = r.fft->max_points;
    if (most < 1 || most > sht_fft::kPoints) return GWEN_EINVAL;
    const int tile = 1 << sht_fft::tile_log2_of((int)most, s.C);
    s.fft_ctiles = (s.C + tile - 1) / tile;
    s.ring_lds_slots = sht_fft::ring_lds_slots((int)most, s.C);
    s.item_blocks = (nlat + sht_fft::kXcds - 1) * (int64_t)s.fft_ctiles;
    if (lat > s.item_blocks) s.item_blocks = lat;
    s.ring_fft = {reinterpret_cast<const sht_fft::RingPlan *>(r.fft->ring_plan),
                  reinterpret_cast<const sht_fft::cpx *>(r.fft->chirp),
                  reinterpret_cast<const sht_fft::cpx *>(r.fft->filter),
                  reinterpret_cast<const sht_fft::cpx *>(r.fft->conv_twiddle)};
  }
  return 0;
}

// items of one pass: what the workspace holds, and what a grid of 2^31 - 1 blocks holds
int chunk_items(const Shape &s, size_t workspace_bytes, int64_t batch, int64_t &chunk) {
  if (s.item_blocks > INT32_MAX) return GWEN_ERANGE;
  chunk = (int64_t)(workspace_bytes / (size_t)s.item_bytes);
  if (chunk < 1) return GWEN_ENOSPACE;
  const int64_t by_grid = INT32_MAX / s.item_blocks;
  if (chunk > by_grid) chunk = by_grid;
  if (chunk > batch) chunk = batch;
  return 0;
}

bool is_vector(int op) { return op == GWEN_SHT_OP_VECTOR_ANALYSIS || op == GWEN_SHT_OP_VECTOR_SYNTHESIS; }

// Everything about a call of a valid op that is judged before a HIP call; 0 = fine, with the shape and the items of a
// pass (0 for an empty batch).  The vector transforms have two inputs and two outputs, an adjoint flag and a ring of
// twice the scalar's; the scalar ones do not read in1, out1 or adjoint.  One coefficient tensor of the vector synthesis
// may be NULL.  rings: the tables of a reduced grid (k.nlon is then its longest ring, k.grid and k.longitude are not
// read), or NULL.
int check_call(const gwen_sht_call &k, const Rings *rings, Shape &s, int64_t &chunk) {
  const bool vec = is_vector(k.op), in_optional = k.op == GWEN_SHT_OP_VECTOR_SYNTHESIS;
  int rc = rings ? check_rings_shape(*rings, k.nlat, k.nlon, k.lmax, k.C, s)
                 : check_shape(k.grid, k.nlat, k.nlon, k.lmax, k.C, s, k.longitude);
  if (rc) return rc;
  if (vec) s.item_bytes *= 2;
  if (k.batch < 0 || (k.in_f64 != 0 && k.in_f64 != 1) || (k.out_f64 != 0 && k.out_f64 != 1)) return GWEN_EINVAL;
  if (vec && k.adjoint != 0 && k.adjoint != 1) return GWEN_EINVAL;
  chunk = 0;
  if (k.batch == 0) return 0;
  if (rings && !(rings->nlon && rings->start && gwen_aligned(rings->nlon, 4) && gwen_aligned(rings->start, 8)))
    return GWEN_EINVAL;
  if (rings && rings->fft) {
    const gwen_sht_rings_fft_call &f = *rings->fft;
    if (!f.ring_plan || !f.chirp || !f.filter || !f.conv_twiddle) return GWEN_EINVAL;
    if (!gwen_aligned(f.ring_plan, 16) || !gwen_aligned(f.chirp, 16) || !gwen_aligned(f.filter, 16) ||
        !gwen_aligned(f.conv_twiddle, 16))
      return GWEN_EINVAL;
  }
  const void *in1 = vec ? k.in1 : k.in0, *out1 = vec ? k.out1 : k.out0;
  if (in_optional ? !k.in0 && !in1 : !k.in0 || !in1) return GWEN_EINVAL;
  if (!k.out0 || !out1 || !k.nodes || !k.twiddle || !k.seed || !k.workspace) return GWEN_EINVAL;
  const size_t in_size = k.in_f64 ? 8 : 4, out_size = k.out_f64 ? 8 : 4;
  if (!gwen_aligned(k.in0, in_size) || !gwen_aligned(in1, in_size) || !gwen_aligned(k.out0, out_size) ||
      !gwen_aligned(out1, out_size) || !gwen_aligned(k.nodes, 16) || !gwen_aligned(k.twiddle, 16) ||
      !gwen_aligned(k.seed, 8) || !gwen_aligned(k.workspace, 8))
    return GWEN_EINVAL;
  // lat_w's alignment is judged before the workspace's size by the vector transforms and after it by the scalar ones, as
  // each has done since it was written: a caller with both wrong gets the code it has always got.
  const bool lat_w_ok = !k.lat_w || gwen_aligned(k.lat_w, 8);
  if (vec && !lat_w_ok) return GWEN_EINVAL;
  rc = chunk_items(s, k.workspace_bytes, k.batch, chunk);
  return rc ? rc : lat_w_ok ? 0 : GWEN_EINVAL;
}

// A launch may ask for 64 KB of dynamic LDS as it is; above that the kernel's limit is raised first.
template <typename Kernel>
int allow_dynamic_lds(Kernel *kernel, size_t lds) {
  if (lds > 64 * 1024)
    GWEN_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds));
  return 0;
}

// the grid and the dynamic LDS of an FFT longitude kernel over `rings` rings
template <typename Kernel>
int fft_launch(const Shape &s, Kernel *kernel, int64_t rings, dim3 &grid, size_t &lds) {
  grid = dim3((unsigned)sht_fft::grid_blocks(rings, s.fft_ctiles));
  lds = sht_fft::lds_bytes(s.fft);
  return allow_dynamic_lds(kernel, lds);
}

// the grid and the dynamic LDS of a ragged FFT longitude kernel over nb items
template <typename Kernel>
int rings_fft_launch(const Shape &s, Kernel *kernel, int64_t nb, dim3 &grid, size_t &lds) {
  grid = dim3((unsigned)sht_fft::grid_blocks(nb * s.nlat, s.fft_ctiles));      // <= nb item_blocks
  lds = sizeof(sht_fft::cpx) * (size_t)s.ring_lds_slots;
  return allow_dynamic_lds(kernel, lds);
}

// The longitude stage of nb items: the direct sums or the FFT, as the shape says.
template <typename TIn>
int lon_fwd(const Shape &s, const TIn *x, const double *tw, double *ring, int64_t nb, hipStream_t st) {
  const int64_t rows = nb * s.nlat * s.C;
  if (s.ring_fft.plan) {
    dim3 grid;
    size_t lds;
    if (const int rc = rings_fft_launch(s, &sht_fft::k_sht_rings_lon_fft_fwd<TIn>, nb, grid, lds)) return rc;
    sht_fft::k_sht_rings_lon_fft_fwd<TIn><<<grid, dim3(sht_fft::kThreads), lds, st>>>(
        x, reinterpret_cast<const sht_fft::cpx *>(tw), s.ring_nlon, s.ring_start, s.ring_fft, ring, nb * s.nlat,
        s.points, s.nlat, (int)nb, s.L, s.C, s.fft_ctiles, s.ring_lds_slots);
  } else if (s.ring_nlon) {
    const int64_t lanes = nb * s.C, ltiles = (lanes + 63) / 64;      // nlat ltiles mtiles <= nb item_blocks
    k_sht_rings_lon_fwd<TIn><<<dim3((unsigned)(s.nlat * ltiles * s.mtiles)), dim3(kThreads), 0, st>>>(
        x, reinterpret_cast<const dpair *>(tw), s.ring_nlon, s.ring_start, ring, lanes, s.points, s.nlat, s.L, s.C,
        s.mtiles, (int)ltiles);
  } else if (s.longitude == GWEN_SHT_LON_DIRECT) {
    k_sht_lon_fwd<TIn><<<dim3((unsigned)((rows + 63) / 64 * s.mtiles)), dim3(kThreads), 0, st>>>(
        x, reinterpret_cast<const dpair *>(tw), ring, rows, s.nlon, s.L, s.C, s.mtiles);
  } else {
    dim3 grid;
    size_t lds;
    if (const int rc = fft_launch(s, &sht_fft::k_sht_lon_fft_fwd<TIn>, nb * s.nlat, grid, lds)) return rc;
    sht_fft::k_sht_lon_fft_fwd<TIn><<<grid, dim3(sht_fft::kThreads), lds, st>>>(
        x, reinterpret_cast<const sht_fft::cpx *>(tw), ring, nb * s.nlat, s.nlon, s.L, s.C, s.fft_ctiles, s.fft);
  }
  GWEN_LAUNCH_CHECK();
  return 0;
}

template <typename TOut>
int lon_inv(const Shape &s, const double *ring, const double *tw, const double *lat_w, TOut *x, int64_t nb,
            hipStream_t st) {
  const int64_t rows = nb * s.nlat * s.C;
  if (s.ring_fft.plan) {
    dim3 grid;
    size_t lds;
    if (const int rc = rings_fft_launch(s, &sht_fft::k_sht_rings_lon_fft_inv<TOut>, nb, grid, lds)) return rc;
    sht_fft::k_sht_rings_lon_fft_inv<TOut><<<grid, dim3(sht_fft::kThreads), lds, st>>>(
        ring, reinterpret_cast<const sht_fft::cpx *>(tw), s.ring_nlon, s.ring_start, s.ring_fft, lat_w, x, nb * s.nlat,
        s.points, s.nlat, (int)nb, s.L, s.C, s.fft_ctiles, s.ring_lds_slots);
  } else if (s.ring_nlon) {
    const int64_t lanes = nb * s.C, ltiles = (lanes + 63) / 64;
    k_sht_rings_lon_inv<TOut><<<dim3((unsigned)(s.nlat * ltiles * s.itiles)), dim3(kThreads), 0, st>>>(
        ring, reinterpret_cast<const dpair *>(tw), s.ring_nlon, s.ring_start, lat_w, x, lanes, s.points, s.nlat, s.L,
        s.C, s.itiles, (int)ltiles);
  } else if (s.longitude == GWEN_SHT_LON_DIRECT) {
    k_sht_lon_inv<TOut><<<dim3((unsigned)((rows + 63) / 64 * s.itiles)), dim3(kThreads), 0, st>>>(
        ring, reinterpret_cast<const dpair *>(tw), lat_w, x, rows, s.nlat, s.nlon, s.L, s.C, s.itiles);
  } else {
    dim3 grid;
    size_t lds;
    if (const int rc = fft_launch(s, &sht_fft::k_sht_lon_fft_inv<TOut>, nb * s.nlat, grid, lds)) return rc;
    sht_fft::k_sht_lon_fft_inv<TOut><<<grid, dim3(sht_fft::kThreads), lds, st>>>(
        ring, reinterpret_cast<const sht_fft::cpx *>(tw), lat_w, x, nb * s.nlat, s.nlat, s.nlon, s.L, s.C, s.fft_ctiles,
        s.fft);
  }
  GWEN_LAUNCH_CHECK();
  return 0;
}

// the dynamic LDS of k_sht_lat_fwd (V = false) and of k_vsht_lat_fwd
size_t lat_fwd_lds(bool V, int nlat) {
  const size_t NT = V ? 2 : 1;
  return sizeof(double) * (2 * (size_t)nlat + NT * kLT * kJT + kJT * 2 * NT * kCT + (2 + V) * kLT);
}

// The transforms of a checked call, `chunk` items a pass: one field (V = false) or two.  The ring of a pass of nb items
// is [1 + V, nb, nlat, 2 lmax + 1, C]: u's first, then v's.
template <bool V, typename TIn, typename TOut>
int analysis(const Shape &s, const gwen_sht_call &k, int64_t chunk) {
  hipStream_t st = gwen_stream(k.stream);
  const dpair *nodes = reinterpret_cast<const dpair *>(k.nodes);
  const TIn *in[2] = {static_cast<const TIn *>(k.in0), static_cast<const TIn *>(k.in1)};
  TOut *out0 = static_cast<TOut *>(k.out0), *out1 = static_cast<TOut *>(k.out1);
  double *ring = static_cast<double *>(k.workspace);
  const size_t lds = lat_fwd_lds(V, s.nlat);
  if (const int rc = V ? allow_dynamic_lds(&k_vsht_lat_fwd<TOut>, lds) : allow_dynamic_lds(&k_sht_lat_fwd<TOut>, lds))
    return rc;
  const int64_t TC = (int64_t)(s.L + 1) * (s.L + 1) * s.C, item = (int64_t)s.nlat * (2 * s.L + 1) * s.C;
  for (int64_t b0 = 0; b0 < k.batch; b0 += chunk) {
    const int64_t nb = k.batch - b0 < chunk ? k.batch - b0 : chunk;
    for (int f = 0; f <= V; ++f)
      if (const int rc = lon_fwd(s, in[f] + b0 * s.points * s.C, k.twiddle, ring + f * nb * item, nb, st)) return rc;
    const dim3 grid((unsigned)(nb * s.ctiles * (s.L + 1)));
    if constexpr (V)
      k_vsht_lat_fwd<TOut><<<grid, dim3(kThreads), lds, st>>>(ring, ring + nb * item, nodes, k.lat_w, k.seed,
                                                              out0 + b0 * TC, out1 + b0 * TC, s.nlat, s.L, s.C, s.ctiles,
                                                              k.adjoint);
    else
      k_sht_lat_fwd<TOut><<<grid, dim3(kThreads), lds, st>>>(ring, nodes, k.lat_w, k.seed, out0 + b0 * TC, s.nlat, s.L,
                                                             s.C, s.ctiles);
    GWEN_LAUNCH_CHECK();
  }
  return 0;
}

template <bool V, typename TIn, typename TOut>
int synthesis(const Shape &s, const gwen_sht_call &k, int64_t chunk) {
  hipStream_t st = gwen_stream(k.stream);
  const dpair *nodes = reinterpret_cast<const dpair *>(k.nodes);
  const TIn *in0 = static_cast<const TIn *>(k.in0), *in1 = static_cast<const TIn *>(k.in1);
  TOut *out[2] = {static_cast<TOut *>(k.out0), static_cast<TOut *>(k.out1)};
  double *ring = static_cast<double *>(k.workspace);
  const int64_t TC = (int64_t)(s.L + 1) * (s.L + 1) * s.C, item = (int64_t)s.nlat * (2 * s.L + 1) * s.C;
  for (int64_t b0 = 0; b0 < k.batch; b0 += chunk) {
    const int64_t nb = k.batch - b0 < chunk ? k.batch - b0 : chunk;
    const dim3 grid((unsigned)(nb * s.ctiles * (s.L + 1) * s.jtiles));
    if constexpr (V)
      k_vsht_lat_inv<TIn><<<grid, dim3(kThreads), 0, st>>>(in0 ? in0 + b0 * TC : nullptr, in1 ? in1 + b0 * TC : nullptr,
                                                           nodes, k.seed, ring, ring + nb * item, s.nlat, s.L, s.C,
                                                           s.ctiles, s.jtiles, k.adjoint);
    else
      k_sht_lat_inv<TIn><<<grid, dim3(kThreads), 0, st>>>(in0 + b0 * TC, nodes, k.seed, ring, s.nlat, s.L, s.C, s.ctiles,
                                                          s.jtiles);
    GWEN_LAUNCH_CHECK();
    for (int f = 0; f <= V; ++f)
      if (const int rc = lon_inv(s, ring + f * nb * item, k.twiddle, k.lat_w, out[f] + b0 * s.points * s.C, nb, st))
        return rc;
  }
  return 0;
}

// gwen_sht_transform and gwen_sht_rings_transform: the checks, then the op in the call's two dtypes
int transform(const gwen_sht_call &k, const Rings *rings) {
  if (k.op < GWEN_SHT_OP_ANALYSIS || k.op > GWEN_SHT_OP_VECTOR_SYNTHESIS) return GWEN_EINVAL;
  Shape s;
  int64_t chunk;
  const int rc = check_call(k, rings, s, chunk);
  if (rc || k.batch == 0) return rc;
  const auto run = [&](auto in, auto out) {
    using TIn = decltype(in);
    using TOut = decltype(out);
    switch (k.op) {
      case GWEN_SHT_OP_ANALYSIS: return analysis<false, TIn, TOut>(s, k, chunk);
      case GWEN_SHT_OP_SYNTHESIS: return synthesis<false, TIn, TOut>(s, k, chunk);
      case GWEN_SHT_OP_VECTOR_ANALYSIS: return analysis<true, TIn, TOut>(s, k, chunk);
      default: return synthesis<true, TIn, TOut>(s, k, chunk);
    }
  };
  if (k.in_f64) return k.out_f64 ? run(double(), double()) : run(double(), float());
  return k.out_f64 ? run(float(), double()) : run(float(), float());
}

// the fields that a reduced grid's call shares with gwen_sht_call; nlon is its longest ring
gwen_sht_call rings_as_call(const gwen_sht_rings_call *call) {
  gwen_sht_call k = {};
  k.op = call->op;
  k.longitude = GWEN_SHT_LON_DIRECT;
  k.in0 = call->in0;
  k.in1 = call->in1;
  k.in_f64 = call->in_f64;
  k.out0 = call->out0;
  k.out1 = call->out1;
  k.out_f64 = call->out_f64;
  k.nodes = call->nodes;
  k.lat_w = call->lat_w;
  k.twiddle = call->twiddle;
  k.seed = call->seed;
  k.grid = GWEN_SHT_GAUSS;
  k.adjoint = call->adjoint;
  k.batch = call->batch;
  k.nlat = call->nlat;
  k.nlon = call->max_nlon;
  k.lmax = call->lmax;
  k.C = call->C;
  k.workspace = call->workspace;
  k.workspace_bytes = call->workspace_bytes;
  k.stream = call->stream;
  return k;
}

}  // namespace

extern "C" {

int gwen_sht_fft_supported(int64_t nlon) { return sht_fft::supported(nlon) ? 1 : 0; }

int gwen_sht_transform(const gwen_sht_call *call) {
  if (!call) return GWEN_EINVAL;
  return transform(*call, nullptr);
}

int gwen_sht_rings_transform(const gwen_sht_rings_call *call) {
  if (!call) return GWEN_EINVAL;
  const Rings rings = {call->ring_nlon, call->ring_start, call->points, nullptr};
  return transform(rings_as_call(call), &rings);
}

int gwen_sht_ring_fft_plan(int64_t nlon, int64_t *n, int64_t *M) {
  if (!n || !M || nlon < 1 || nlon > 2 * (int64_t)sht_fft::kPoints) return 0;
  *n = nlon % 2 == 0 ? nlon / 2 : nlon;
  *M = 0;
  if (sht_fft::supported(nlon)) return sht_fft::kRingMixed;
  int64_t m = 2 * *n - 1;
  while (m <= sht_fft::kPoints && !sht_fft::supported(m)) ++m;
  if (m > sht_fft::kPoints) return 0;
  *M = m;
  return sht_fft::kRingBluestein;
}

int gwen_sht_rings_fft_transform(const gwen_sht_rings_fft_call *call) {
  if (!call) return GWEN_EINVAL;
  const Rings rings = {call->rings.ring_nlon, call->rings.ring_start, call->rings.points, call};
  return transform(rings_as_call(&call->rings), &rings);
}

int64_t gwen_sht_rings_workspace_bytes(int vector, int64_t nlat, int64_t points, int64_t max_nlon, int64_t lmax,
                                       int64_t C) {
  Shape s;
  const Rings rings = {nullptr, nullptr, points, nullptr};
  if ((vector != 0 && vector != 1) || check_rings_shape(rings, nlat, max_nlon, lmax, C, s)) return 0;
  return vector ? 2 * s.item_bytes : s.item_bytes;
}

int64_t gwen_sht_vector_workspace_bytes(int grid, int64_t nlat, int64_t nlon, int64_t lmax, int64_t C) {
  Shape s;
  return check_shape(grid, nlat, nlon, lmax, C, s) ? 0 : 2 * s.item_bytes;
}

int gwen_sht_vector_analysis(const void *u, const void *v, int x_f64, void *vort, void *div, int coef_f64,
                             const double *nodes, const double *lat_w, const double *twiddle, const double *seed,
                             int grid, int64_t batch, int64_t nlat, int64_t nlon, int64_t lmax, int64_t C, int adjoint,
                             void *workspace, size_t workspace_bytes, gwen_stream_t stream) {
  gwen_sht_call k = {};
  k.op = GWEN_SHT_OP_VECTOR_ANALYSIS;
  k.longitude = GWEN_SHT_LON_DIRECT;
  k.in0 = u;
  k.in1 = v;
  k.in_f64 = x_f64;
  k.out0 = vort;
  k.out1 = div;
  k.out_f64 = coef_f64;
  k.nodes = nodes;
  k.lat_w = lat_w;
  k.twiddle = twiddle;
  k.seed = seed;
  k.grid = grid;
  k.adjoint = adjoint;
  k.batch = batch;
  k.nlat = nlat;
  k.nlon = nlon;
  k.lmax = lmax;
  k.C = C;
  k.workspace = workspace;
  k.workspace_bytes = workspace_bytes;
  k.stream = stream;
  return transform(k, nullptr);
}

int gwen_sht_vector_synthesis(const void *vort, const void *div, int coef_f64, void *u, void *v, int x_f64,
                              const double *nodes, const double *lat_w, const double *twiddle, const double *seed,
                              int grid, int64_t batch, int64_t nlat, int64_t nlon, int64_t lmax, int64_t C, int adjoint,
                              void *workspace, size_t workspace_bytes, gwen_stream_t stream) {
  gwen_sht_call k = {};
  k.op = GWEN_SHT_OP_VECTOR_SYNTHESIS;
  k.longitude = GWEN_SHT_LON_DIRECT;
  k.in0 = vort;
  k.in1 = div;
  k.in_f64 = coef_f64;
  k.out0 = u;
  k.out1 = v;
  k.out_f64 = x_f64;
  k.nodes = nodes;
  k.lat_w = lat_w;
  k.twiddle = twiddle;
  k.seed = seed;
  k.grid = grid;
  k.adjoint = adjoint;
  k.batch = batch;
  k.nlat = nlat;
  k.nlon = nlon;
  k.lmax = lmax;
  k.C = C;
  k.workspace = workspace;
  k.workspace_bytes = workspace_bytes;
  k.stream = stream;
  return transform(k, nullptr);
}

int64_t gwen_sht_workspace_bytes(int grid, int64_t nlat, int64_t nlon, int64_t lmax, int64_t C) {
  Shape s;
  return check_shape(grid, nlat, nlon, lmax, C, s) ? 0 : s.item_bytes;
}

int gwen_sht_analysis(const void *x, int x_f64, void *coef, int coef_f64, const double *nodes, const double *lat_w,
                      const double *twiddle, const double *seed, int grid, int64_t batch, int64_t nlat, int64_t nlon,
                      int64_t lmax, int64_t C, void *workspace, size_t workspace_bytes, gwen_stream_t stream) {
  gwen_sht_call k = {};                                   // in1, out1 and adjoint are not the scalar transforms'
  k.op = GWEN_SHT_OP_ANALYSIS;
  k.longitude = GWEN_SHT_LON_DIRECT;
  k.in0 = x;
  k.in_f64 = x_f64;
  k.out0 = coef;
  k.out_f64 = coef_f64;
  k.nodes = nodes;
  k.lat_w = lat_w;
  k.twiddle = twiddle;
  k.seed = seed;
  k.grid = grid;
  k.batch = batch;
  k.nlat = nlat;
  k.nlon = nlon;
  k.lmax = lmax;
  k.C = C;
  k.workspace = workspace;
  k.workspace_bytes = workspace_bytes;
  k.stream = stream;
  return transform(k, nullptr);
}

int gwen_sht_synthesis(const void *coef, int coef_f64, void *x, int x_f64, const double *nodes, const double *lat_w,
                       const double *twiddle, const double *seed, int grid, int64_t batch, int64_t nlat, int64_t nlon,
                       int64_t lmax, int64_t C, void *workspace, size_t workspace_bytes, gwen_stream_t stream) {
  gwen_sht_call k = {};
  k.op = GWEN_SHT_OP_SYNTHESIS;
  k.longitude = GWEN_SHT_LON_DIRECT;
  k.in0 = coef;
  k.in_f64 = coef_f64;
  k.out0 = x;
  k.out_f64 = x_f64;
  k.nodes = nodes;
  k.lat_w = lat_w;
  k.twiddle = twiddle;
  k.seed = seed;
  k.grid = grid;
  k.batch = batch;
  k.nlat = nlat;
  k.nlon = nlon;
  k.lmax = lmax;
  k.C = C;
  k.workspace = workspace;
  k.workspace_bytes = workspace_bytes;
  k.stream = stream;
  return transform(k, nullptr);
}

int gwen_sht_power_f64(const double *coef, double *power, int64_t batch, int64_t lmax, int64_t C,
                       gwen_stream_t stream) {
  if (batch < 0 || lmax < 0 || lmax > kLMax || C < 1) return GWEN_EINVAL;
  if (C > INT32_MAX) return GWEN_ERANGE;
  if (batch == 0) return 0;
  if (!coef || !power || !gwen_aligned(coef, 8) || !gwen_aligned(power, 8)) return GWEN_EINVAL;
  if (batch > INT64_MAX / ((lmax + 1) * C)) return GWEN_ERANGE;
  const int64_t total = batch * (lmax + 1) * C;
  const int64_t blocks = (total + kThreads - 1) / kThreads;
  if (blocks > INT32_MAX) return GWEN_ERANGE;
  k_sht_power<<<dim3((unsigned)blocks), dim3(kThreads), 0, gwen_stream(stream)>>>(coef, power, total, (int)lmax, (int)C);
  GWEN_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
