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
#include "common.h"

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

// a, b of Pbar_l^m = a (mu Pbar_{l-1}^m - b Pbar_{l-2}^m), l > m (l = m + 1: a = sqrt(2m + 3), b = 0)
__device__ __forceinline__ void recurrence_coefficients(int l, int m, double &a, double &b) {
  const double dl = (double)l, dm = (double)m, dl1 = (double)(l - 1);
  a = sqrt((4.0 * dl * dl - 1.0) / (dl * dl - dm * dm));
  b = sqrt((dl1 * dl1 - dm * dm) / (4.0 * dl1 * dl1 - 1.0));
}

// The longitude sums.  A lane owns one (ring, channel) row of x -- rows run over (item, latitude, channel), so every lane
// works whatever C is -- and a wave owns 16 orders m: the orders, their table indices (m i) mod nlon and the twiddles are
// wave-uniform (scalar registers, scalar loads), and the vector unit issues little but the 32 fma of a longitude.
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
  int mk[kLonK], idx[kLonK];
  double ac[kLonK], as[kLonK];
#pragma unroll
  for (int k = 0; k < kLonK; ++k) {
    mk[k] = m0 + k <= L ? m0 + k : 0;                     // an order past lmax walks order 0 and is not stored
    idx[k] = 0;
    ac[k] = 0.0;
    as[k] = 0.0;
  }
  const TIn *xp = x + row * (int64_t)nlon * C + c;
#pragma unroll 2
  for (int i = 0; i < nlon; ++i) {
    const double xv = (double)xp[(int64_t)i * C];
#pragma unroll
    for (int k = 0; k < kLonK; ++k) {
      const dpair t = tw[idx[k]];
      ac[k] = fma(xv, t.x, ac[k]);
      as[k] = fma(xv, t.y, as[k]);
      idx[k] += mk[k];
      if (idx[k] >= nlon) idx[k] -= nlon;
    }
  }
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

// Block (item, channel tile, order m): all latitudes, all degrees l >= m.  Dynamic LDS: two recurrence values per
// latitude, the Legendre tile (column (j + l) & 63: conflict-free for the writer's 64 latitudes and for the readers' 4
// degrees a wave), the ring tile and the recurrence coefficients of the tile's degrees.
template <typename TOut>
__global__ __launch_bounds__(kThreads) void k_sht_lat_fwd(const double *__restrict__ ring, const dpair *__restrict__ nodes,
                                                          const double *__restrict__ lat_w,
                                                          const double *__restrict__ seed, TOut *__restrict__ coef,
                                                          int nlat, int L, int C, int ctiles) {
  extern __shared__ double smem[];
  double *st1 = smem;                                     // [nlat]  Pbar_{l-1}^m at the start of a degree tile
  double *st2 = st1 + nlat;                               // [nlat]  Pbar_{l-2}^m
  double *pt = st2 + nlat;                                // [kLT][kJT]
  double *ft = pt + kLT * kJT;                            // [kJT][2][kCT]
  double *ca = ft + kJT * 2 * kCT;                        // [kLT]
  double *cb = ca + kLT;                                  // [kLT]
  const int tid = threadIdx.x, cl = tid & (kCT - 1), lg = tid >> 4;
  int64_t blk = blockIdx.x;
  const int m = (int)(blk % (L + 1));
  blk /= (L + 1);
  const int ct = (int)(blk % ctiles);
  const int64_t item = blk / ctiles;
  const int c = ct * kCT + cl;
  const int64_t T = (int64_t)(L + 1) * (L + 1);
  const double sm = seed[m];
  for (int j = tid; j < nlat; j += kThreads) {
    st1[j] = sm * powi(nodes[j].y, m);
    st2[j] = 0.0;
  }
  const double *fr = ring + item * (int64_t)nlat * (2 * L + 1) * C;
  for (int l0 = m; l0 <= L; l0 += kLT) {
    const int nl = L - l0 + 1 < kLT ? L - l0 + 1 : kLT;
    __syncthreads();                                      // the tile before is done with ca, cb (and st1, st2 are set)
    if (tid < nl && l0 + tid > m) {
      double a, b;
      recurrence_coefficients(l0 + tid, m, a, b);
      ca[tid] = a;
      cb[tid] = b;
    }
    double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (int j0 = 0; j0 < nlat; j0 += kJT) {
      __syncthreads();
      if (tid < kJT) {
        const int j = j0 + tid;
        if (j < nlat) {
          double p1 = st1[j], p2 = st2[j];
          const double mu = nodes[j].x, w = lat_w ? lat_w[j] : 1.0;
          for (int t = 0; t < nl; ++t) {
            if (l0 + t > m) {
              const double p = ca[t] * (mu * p1 - cb[t] * p2);
              p2 = p1;
              p1 = p;
            }
            pt[t * kJT + ((tid + t) & (kJT - 1))] = p1 * w;
          }
          st1[j] = p1;
          st2[j] = p2;
        } else {
          for (int t = 0; t < nl; ++t) pt[t * kJT + ((tid + t) & (kJT - 1))] = 0.0;
        }
      }
#pragma unroll
      for (int r = 0; r < kJT * 2 * kCT / kThreads; ++r) {
        const int e = tid + kThreads * r, cc = e & (kCT - 1), kk = (e >> 4) & 1, jj = e >> 5;
        const int j = j0 + jj, gc = ct * kCT + cc;
        ft[e] = j < nlat && gc < C ? fr[((int64_t)j * (2 * L + 1) + (kk ? L - m : L + m)) * C + gc] : 0.0;
      }
      __syncthreads();
      const int nj = nlat - j0 < kJT ? nlat - j0 : kJT;
      for (int jj = 0; jj < nj; ++jj) {
        const double fc = ft[(jj * 2 + 0) * kCT + cl], fs = ft[(jj * 2 + 1) * kCT + cl];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int t = lg + 16 * r;
          const double p = t < nl ? pt[t * kJT + ((jj + t) & (kJT - 1))] : 0.0;
          acc[r][0] = fma(p, fc, acc[r][0]);
          acc[r][1] = fma(p, fs, acc[r][1]);
        }
      }
    }
    if (c < C) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int l = l0 + lg + 16 * r;
        if (l > L) continue;
        TOut *o = coef + (item * T + (int64_t)l * l + l) * C + c;
        o[(int64_t)m * C] = (TOut)acc[r][0];
        if (m > 0) o[-(int64_t)m * C] = (TOut)acc[r][1];
      }
    }
  }
}

// Block (item, channel tile, order m, 64 latitudes): the recurrence lives in the registers of the block's first 64
// threads; thread (channel, 4 latitudes) sums over the degrees.
template <typename TIn>
__global__ __launch_bounds__(kThreads) void k_sht_lat_inv(const TIn *__restrict__ coef, const dpair *__restrict__ nodes,
                                                          const double *__restrict__ seed, double *__restrict__ ring,
                                                          int nlat, int L, int C, int ctiles, int jtiles) {
  __shared__ double pt[kLT * kJT];
  __shared__ double ctile[kLT * 2 * kCT];
  __shared__ double ca[kLT], cb[kLT];
  const int tid = threadIdx.x, cl = tid & (kCT - 1), jg = tid >> 4;
  int64_t blk = blockIdx.x;
  const int jt = (int)(blk % jtiles);
  blk /= jtiles;
  const int m = (int)(blk % (L + 1));
  blk /= (L + 1);
  const int ct = (int)(blk % ctiles);
  const int64_t item = blk / ctiles;
  const int c = ct * kCT + cl;
  const int64_t T = (int64_t)(L + 1) * (L + 1);
  const int j0 = jt * kJT;
  const int jmine = j0 + tid;
  double p1 = 0.0, p2 = 0.0, mu = 0.0;
  if (tid < kJT && jmine < nlat) {
    p1 = seed[m] * powi(nodes[jmine].y, m);
    mu = nodes[jmine].x;
  }
  double acc[4][2];
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r][0] = acc[r][1] = 0.0;
  const TIn *cf = coef + item * T * C;
  for (int l0 = m; l0 <= L; l0 += kLT) {
    const int nl = L - l0 + 1 < kLT ? L - l0 + 1 : kLT;
    __syncthreads();
    if (tid < nl && l0 + tid > m) {
      double a, b;
      recurrence_coefficients(l0 + tid, m, a, b);
      ca[tid] = a;
      cb[tid] = b;
    }
#pragma unroll
    for (int r = 0; r < kLT * 2 * kCT / kThreads; ++r) {
      const int e = tid + kThreads * r, cc = e & (kCT - 1), kk = (e >> 4) & 1, t = e >> 5;
      const int l = l0 + t, gc = ct * kCT + cc;
      ctile[e] = l <= L && gc < C && !(kk && m == 0)
                     ? (double)cf[((int64_t)l * l + l + (kk ? -m : m)) * C + gc] : 0.0;
    }
    __syncthreads();
    if (tid < kJT) {
      for (int t = 0; t < nl; ++t) {
        if (l0 + t > m) {
          const double p = ca[t] * (mu * p1 - cb[t] * p2);
          p2 = p1;
          p1 = p;
        }
        pt[t * kJT + ((tid + t) & (kJT - 1))] = p1;
      }
    }
    __syncthreads();
    for (int t = 0; t < nl; ++t) {
      const double cc_ = ctile[(t * 2 + 0) * kCT + cl], cs = ctile[(t * 2 + 1) * kCT + cl];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double p = pt[t * kJT + ((jg + 16 * r + t) & (kJT - 1))];
        acc[r][0] = fma(p, cc_, acc[r][0]);
        acc[r][1] = fma(p, cs, acc[r][1]);
      }
    }
  }
  if (c >= C) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = j0 + jg + 16 * r;
    if (j >= nlat) continue;
    double *o = ring + ((item * nlat + j) * (int64_t)(2 * L + 1) + L) * C + c;
    o[(int64_t)m * C] = acc[r][0];
    if (m > 0) o[-(int64_t)m * C] = acc[r][1];
  }
}

// The longitude synthesis, the same way round: a lane owns one (ring, channel) row, a wave 16 longitudes (wave-uniform
// table indices and twiddles), and every lane sums over the orders.
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
  int step[kLonK], idx[kLonK];
  double acc[kLonK];
#pragma unroll
  for (int k = 0; k < kLonK; ++k) {
    step[k] = i0 + k < nlon ? i0 + k : 0;
    idx[k] = 0;
    acc[k] = 0.0;
  }
  const double *gp = ring + (row * (int64_t)(2 * L + 1) + L) * C + c;
#pragma unroll 2
  for (int m = 0; m <= L; ++m) {
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
  if (r >= rows) return;
  const double w = lat_w ? lat_w[row % nlat] : 1.0;
  TOut *xo = x + row * (int64_t)nlon * C + c;
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

struct Shape {
  int nlat, nlon, L, C, ctiles, mtiles, itiles, jtiles;
  int64_t item_bytes, item_blocks;
};

// sizes only; 0 = fine
int check_shape(int grid, int64_t nlat, int64_t nlon, int64_t lmax, int64_t C, Shape &s) {
  if (grid != GWEN_SHT_EQUIANGULAR && grid != GWEN_SHT_EQUIANGULAR_CENTRED && grid != GWEN_SHT_GAUSS) return GWEN_EINVAL;
  if (nlat < (grid == GWEN_SHT_EQUIANGULAR ? 2 : 1) || nlat > kMaxLat || nlon < 1 || C < 1) return GWEN_EINVAL;
  if (lmax < 0 || lmax > kLMax) return GWEN_EINVAL;
  if (lmax > (grid == GWEN_SHT_GAUSS ? nlat - 1 : (nlat - 1) / 2)) return GWEN_EINVAL;
  if (nlon < 2 * lmax + 1) return GWEN_EINVAL;
  if (nlat * nlon > INT32_MAX || C > INT32_MAX) return GWEN_ERANGE;      // (lmax + 1)^2 <= 2^20
  s.nlat = (int)nlat;
  s.nlon = (int)nlon;
  s.L = (int)lmax;
  s.C = (int)C;
  s.ctiles = (int)((C + kCT - 1) / kCT);
  s.mtiles = (s.L + 4 * kLonK) / (4 * kLonK);
  s.itiles = (s.nlon + 4 * kLonK - 1) / (4 * kLonK);
  s.jtiles = (s.nlat + kJT - 1) / kJT;
  s.item_bytes = nlat * (2 * lmax + 1) * C * (int64_t)sizeof(double);
  const int64_t lon = ((nlat * C + 63) / 64 + 1) * (int64_t)(s.mtiles > s.itiles ? s.mtiles : s.itiles);
  const int64_t lat = s.ctiles * (lmax + 1) * (int64_t)s.jtiles;
  s.item_blocks = lon > lat ? lon : lat;
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

size_t lat_fwd_lds(int nlat) { return sizeof(double) * (2 * (size_t)nlat + kLT * kJT + kJT * 2 * kCT + 2 * kLT); }

template <typename TIn, typename TOut>
int analysis(const Shape &s, const TIn *x, TOut *coef, const double *nodes, const double *lat_w, const double *tw,
             const double *seed, int64_t batch, int64_t chunk, double *ring, hipStream_t st) {
  const size_t lds = lat_fwd_lds(s.nlat);
  if (lds > 64 * 1024)
    GWEN_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sht_lat_fwd<TOut>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int64_t T = (int64_t)(s.L + 1) * (s.L + 1);
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nb = batch - b0 < chunk ? batch - b0 : chunk;
    const int64_t rows = nb * s.nlat * s.C;
    k_sht_lon_fwd<TIn><<<dim3((unsigned)((rows + 63) / 64 * s.mtiles)), dim3(kThreads), 0, st>>>(
        x + b0 * s.nlat * (int64_t)s.nlon * s.C, reinterpret_cast<const dpair *>(tw), ring, rows, s.nlon, s.L, s.C,
        s.mtiles);
    GWEN_LAUNCH_CHECK();
    k_sht_lat_fwd<TOut><<<dim3((unsigned)(nb * s.ctiles * (s.L + 1))), dim3(kThreads), lds, st>>>(
        ring, reinterpret_cast<const dpair *>(nodes), lat_w, seed, coef + b0 * T * s.C, s.nlat, s.L, s.C, s.ctiles);
    GWEN_LAUNCH_CHECK();
  }
  return 0;
}

template <typename TIn, typename TOut>
int synthesis(const Shape &s, const TIn *coef, TOut *x, const double *nodes, const double *lat_w, const double *tw,
              const double *seed, int64_t batch, int64_t chunk, double *ring, hipStream_t st) {
  const int64_t T = (int64_t)(s.L + 1) * (s.L + 1);
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nb = batch - b0 < chunk ? batch - b0 : chunk;
    k_sht_lat_inv<TIn><<<dim3((unsigned)(nb * s.ctiles * (s.L + 1) * s.jtiles)), dim3(kThreads), 0, st>>>(
        coef + b0 * T * s.C, reinterpret_cast<const dpair *>(nodes), seed, ring, s.nlat, s.L, s.C, s.ctiles, s.jtiles);
    GWEN_LAUNCH_CHECK();
    const int64_t rows = nb * s.nlat * s.C;
    k_sht_lon_inv<TOut><<<dim3((unsigned)((rows + 63) / 64 * s.itiles)), dim3(kThreads), 0, st>>>(
        ring, reinterpret_cast<const dpair *>(tw), lat_w, x + b0 * s.nlat * (int64_t)s.nlon * s.C, rows, s.nlat, s.nlon,
        s.L, s.C, s.itiles);
    GWEN_LAUNCH_CHECK();
  }
  return 0;
}

int check_call(const void *a, int a_f64, const void *b, int b_f64, const double *nodes, const double *tw,
               const double *seed, int grid, int64_t batch, int64_t nlat, int64_t nlon, int64_t lmax, int64_t C,
               const void *workspace, size_t workspace_bytes, Shape &s, int64_t &chunk) {
  const int rc = check_shape(grid, nlat, nlon, lmax, C, s);
  if (rc) return rc;
  if (batch < 0 || (a_f64 != 0 && a_f64 != 1) || (b_f64 != 0 && b_f64 != 1)) return GWEN_EINVAL;
  chunk = 0;
  if (batch == 0) return 0;
  if (!a || !b || !nodes || !tw || !seed || !workspace) return GWEN_EINVAL;
  if (!gwen_aligned(a, a_f64 ? 8 : 4) || !gwen_aligned(b, b_f64 ? 8 : 4) || !gwen_aligned(nodes, 16) ||
      !gwen_aligned(tw, 16) || !gwen_aligned(seed, 8) || !gwen_aligned(workspace, 8))
    return GWEN_EINVAL;
  return chunk_items(s, workspace_bytes, batch, chunk);
}

}  // namespace

extern "C" {

int64_t gwen_sht_workspace_bytes(int grid, int64_t nlat, int64_t nlon, int64_t lmax, int64_t C) {
  Shape s;
  return check_shape(grid, nlat, nlon, lmax, C, s) ? 0 : s.item_bytes;
}

int gwen_sht_analysis(const void *x, int x_f64, void *coef, int coef_f64, const double *nodes, const double *lat_w,
                      const double *twiddle, const double *seed, int grid, int64_t batch, int64_t nlat, int64_t nlon,
                      int64_t lmax, int64_t C, void *workspace, size_t workspace_bytes, gwen_stream_t stream) {
  Shape s;
  int64_t chunk;
  const int rc = check_call(x, x_f64, coef, coef_f64, nodes, twiddle, seed, grid, batch, nlat, nlon, lmax, C, workspace,
                            workspace_bytes, s, chunk);
  if (rc || batch == 0) return rc;
  if (lat_w && !gwen_aligned(lat_w, 8)) return GWEN_EINVAL;
  hipStream_t st = gwen_stream(stream);
  double *ring = static_cast<double *>(workspace);
  if (x_f64)
    return coef_f64 ? analysis(s, (const double *)x, (double *)coef, nodes, lat_w, twiddle, seed, batch, chunk, ring, st)
                    : analysis(s, (const double *)x, (float *)coef, nodes, lat_w, twiddle, seed, batch, chunk, ring, st);
  return coef_f64 ? analysis(s, (const float *)x, (double *)coef, nodes, lat_w, twiddle, seed, batch, chunk, ring, st)
                  : analysis(s, (const float *)x, (float *)coef, nodes, lat_w, twiddle, seed, batch, chunk, ring, st);
}

int gwen_sht_synthesis(const void *coef, int coef_f64, void *x, int x_f64, const double *nodes, const double *lat_w,
                       const double *twiddle, const double *seed, int grid, int64_t batch, int64_t nlat, int64_t nlon,
                       int64_t lmax, int64_t C, void *workspace, size_t workspace_bytes, gwen_stream_t stream) {
  Shape s;
  int64_t chunk;
  const int rc = check_call(coef, coef_f64, x, x_f64, nodes, twiddle, seed, grid, batch, nlat, nlon, lmax, C, workspace,
                            workspace_bytes, s, chunk);
  if (rc || batch == 0) return rc;
  if (lat_w && !gwen_aligned(lat_w, 8)) return GWEN_EINVAL;
  hipStream_t st = gwen_stream(stream);
  double *ring = static_cast<double *>(workspace);
  if (coef_f64)
    return x_f64 ? synthesis(s, (const double *)coef, (double *)x, nodes, lat_w, twiddle, seed, batch, chunk, ring, st)
                 : synthesis(s, (const double *)coef, (float *)x, nodes, lat_w, twiddle, seed, batch, chunk, ring, st);
  return x_f64 ? synthesis(s, (const float *)coef, (double *)x, nodes, lat_w, twiddle, seed, batch, chunk, ring, st)
               : synthesis(s, (const float *)coef, (float *)x, nodes, lat_w, twiddle, seed, batch, chunk, ring, st);
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
