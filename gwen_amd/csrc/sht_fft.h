// The longitude stage of the spherical harmonic transforms as an FFT (longitude = GWEN_SHT_LON_FFT): drop-in replacements
// for k_sht_lon_fwd and k_sht_lon_inv of sht.hip, same ring layout, fp64 throughout.
//
// A block owns one latitude ring of one item and a tile of channels; every channel is one transform of its own in LDS
// (nothing is packed across channels or latitudes, so a NaN stays in its (item, channel)).  An even nlon runs the complex
// FFT of length n = nlon / 2 on z[k] = x[2k] + i x[2k + 1] and a split step; an odd nlon runs the full-length complex FFT.
// The FFT is a Stockham autosort, decimation in frequency, radices 4, 2, 3, 5 in the order of the host's plan:
//
//   a stage of radix r at length n' = r m and stride s (n' s = n):   a_k = x[q + s (p + m k)],  k < r
//       y[q + s (r p + j)] = w_n'^(p j) sum_k a_k w_r^(j k),          p < m, q < s, j < r
//
// on ONE buffer: every thread reads the inputs of all its butterflies into registers, the block synchronises, and every
// thread writes.  w_n'^(p j) = w_nlon^(p j s nlon / n) with p j s < n, so every twiddle is an entry of the transforms'
// nlon-entry table, index below nlon without a reduction; the radix-3 and radix-5 butterflies take their constants from
// entries nlon / 3, nlon / 5 and 2 nlon / 5.  The schedule depends on nlon alone, so results are bitwise reproducible.
// The twiddle product is never skipped, not even for the table's entry 0: it is what carries a NaN of one component into
// both.
//
// The same stages serve the rings of a reduced Gaussian grid, a length of its own on every latitude, lengths with other
// prime factors through Bluestein's convolution ("reduced grids" below).
#pragma once

#include "common.h"

namespace sht_fft {

constexpr int kThreads = 256;
constexpr int kPoints = 4096;          // complex points of a block: channel tile x n
constexpr int kMaxTile = 16;
constexpr int kMaxStages = 12;         // 2^11 in radix 4 takes 6, 3^7 takes 7
constexpr int kMaxLon = 4096;
constexpr int kXcds = 8;               // consecutive blocks go to consecutive XCDs: the tiles of a ring share one L2

struct __attribute__((aligned(16))) cpx {
  double x, y;
};

// passed by value; fixed by nlon (and the tile by nlon and C)
struct Plan {
  int n;                               // length of the complex FFT: nlon / 2 (half = 1) or nlon
  int half;
  int tile, tile_log2;                 // channels of a block, a power of two
  int pitch;                           // complex slots of a channel in LDS
  int stages;
  int radix[kMaxStages];
};

// a sequence's element i lives in slot i + i / 8: the stride-2 and stride-4 stores of the first radix-2/4 stage, and the
// power-of-two strides after it, then spread over the banks
__host__ __device__ __forceinline__ int slot(int i) { return i + (i >> 3); }

inline bool supported(int64_t nlon) {
  if (nlon < 1 || nlon > kMaxLon) return false;
  for (int f : {2, 3, 5})
    while (nlon % f == 0) nlon /= f;
  return nlon == 1;
}

// log2 of the channels of a block whose channels take `len` complex points each: the largest power of two that keeps the
// block within kPoints and kMaxTile and is not a whole tile above C.  The launchers and the ragged kernels both ask here.
__host__ __device__ inline int tile_log2_of(int len, int C) {
  int tile = 1, lg = 0;
  while (tile * 2 <= kMaxTile && tile * 2 * len <= kPoints && tile < C) {
    tile *= 2;
    ++lg;
  }
  return lg;
}

// the radices of a complex FFT of length n = 2^a 3^b 5^c: 4, 2, 3, 5 in that order
__host__ __device__ inline void set_stages(Plan &p, int n) {
  constexpr int kRadix[4] = {4, 2, 3, 5};
  p.stages = 0;
  for (int i = 0; i < 4; ++i)
    while (n % kRadix[i] == 0 && p.stages < kMaxStages) {
      p.radix[p.stages++] = kRadix[i];
      n /= kRadix[i];
    }
}

inline Plan make_plan(int nlon, int C) {
  Plan p{};
  p.half = nlon % 2 == 0;
  p.n = p.half ? nlon / 2 : nlon;
  set_stages(p, p.n);
  p.pitch = slot(p.n - 1) + 1;
  p.tile_log2 = tile_log2_of(p.n, C);
  p.tile = 1 << p.tile_log2;
  return p;
}

inline size_t lds_bytes(const Plan &p) { return sizeof(cpx) * (size_t)p.tile * p.pitch; }

__device__ __forceinline__ cpx cmul(cpx a, double wx, double wy) { return {a.x * wx - a.y * wy, a.x * wy + a.y * wx}; }
__device__ __forceinline__ cpx cadd(cpx a, cpx b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cpx csub(cpx a, cpx b) { return {a.x - b.x, a.y - b.y}; }
// i sgn a
template <int SGN>
__device__ __forceinline__ cpx crot(cpx a) {
  return {-(double)SGN * a.y, (double)SGN * a.x};
}

// the r-point DFT with w_r = exp(i SGN 2 pi / r), in place
template <int R, int SGN>
__device__ __forceinline__ void butterfly(cpx (&a)[R], const cpx *__restrict__ tw, int nlon) {
  if constexpr (R == 2) {
    const cpx t = a[1];
    a[1] = csub(a[0], t);
    a[0] = cadd(a[0], t);
  } else if constexpr (R == 4) {
    const cpx s02 = cadd(a[0], a[2]), d02 = csub(a[0], a[2]), s13 = cadd(a[1], a[3]);
    const cpx t = crot<SGN>(csub(a[1], a[3]));
    a[0] = cadd(s02, s13);
    a[1] = cadd(d02, t);
    a[2] = csub(s02, s13);
    a[3] = csub(d02, t);
  } else if constexpr (R == 3) {
    const cpx w = tw[nlon / 3];
    const cpx t1 = cadd(a[1], a[2]), d = csub(a[1], a[2]);
    const cpx m = {a[0].x + w.x * t1.x, a[0].y + w.x * t1.y};
    const cpx t = crot<SGN>(cpx{w.y * d.x, w.y * d.y});
    a[0] = cadd(a[0], t1);
    a[1] = cadd(m, t);
    a[2] = csub(m, t);
  } else {
    static_assert(R == 5, "radix");
    const cpx w1 = tw[nlon / 5], w2 = tw[2 * (nlon / 5)];
    const cpx t1 = cadd(a[1], a[4]), t2 = cadd(a[2], a[3]), t3 = csub(a[1], a[4]), t4 = csub(a[2], a[3]);
    const cpx m1 = {a[0].x + w1.x * t1.x + w2.x * t2.x, a[0].y + w1.x * t1.y + w2.x * t2.y};
    const cpx m2 = {a[0].x + w2.x * t1.x + w1.x * t2.x, a[0].y + w2.x * t1.y + w1.x * t2.y};
    const cpx n1 = crot<SGN>(cpx{w1.y * t3.x + w2.y * t4.x, w1.y * t3.y + w2.y * t4.y});
    const cpx n2 = crot<SGN>(cpx{w2.y * t3.x - w1.y * t4.x, w2.y * t3.y - w1.y * t4.y});
    a[0] = cadd(a[0], cadd(t1, t2));
    a[1] = cadd(m1, n1);
    a[2] = cadd(m2, n2);
    a[3] = csub(m2, n2);
    a[4] = csub(m1, n1);
  }
}

// One stage on every channel of the tile.  m = n' / R; step = s nlon / n, the table stride of p j.
template <int R, int SGN>
__device__ __forceinline__ void stage(cpx *__restrict__ sm, const cpx *__restrict__ tw, const Plan &pl, int nlon, int m,
                                      int s) {
  constexpr int kIter = (kPoints / R + kThreads - 1) / kThreads;
  const unsigned nb = (unsigned)(pl.n / R);            // butterflies of a channel
  const unsigned total = nb << pl.tile_log2;
  const int step = s * (pl.half ? 2 : 1);
  cpx a[kIter][R];
  int base[kIter], pp[kIter], qq[kIter];
#pragma unroll
  for (int it = 0; it < kIter; ++it) {
    const unsigned idx = threadIdx.x + it * kThreads;
    if (idx < total) {
      const unsigned ch = idx / nb, b = idx - ch * nb;
      const unsigned p = b / (unsigned)s, q = b - p * (unsigned)s;
      const cpx *src = sm + ch * pl.pitch;
#pragma unroll
      for (int k = 0; k < R; ++k) a[it][k] = src[slot((int)(q + s * (p + m * k)))];
      base[it] = (int)(ch * pl.pitch);
      pp[it] = (int)p;
      qq[it] = (int)q;
    }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < kIter; ++it) {
    const unsigned idx = threadIdx.x + it * kThreads;
    if (idx < total) {
      const int p = pp[it], q = qq[it];
      butterfly<R, SGN>(a[it], tw, nlon);
      cpx *dst = sm + base[it];
      dst[slot(q + s * R * p)] = a[it][0];
#pragma unroll
      for (int j = 1; j < R; ++j) {
        const cpx w = tw[p * j * step];
        dst[slot(q + s * (R * p + j))] = cmul(a[it][j], w.x, (double)SGN * w.y);
      }
    }
  }
  __syncthreads();
}

template <int SGN>
__device__ __forceinline__ void transform(cpx *__restrict__ sm, const cpx *__restrict__ tw, const Plan &pl, int nlon) {
  int m = pl.n, s = 1;
#pragma unroll 1
  for (int g = 0; g < pl.stages; ++g) {
    const int r = pl.radix[g];
    m /= r;
    if (r == 4) stage<4, SGN>(sm, tw, pl, nlon, m, s);
    else if (r == 2) stage<2, SGN>(sm, tw, pl, nlon, m, s);
    else if (r == 3) stage<3, SGN>(sm, tw, pl, nlon, m, s);
    else stage<5, SGN>(sm, tw, pl, nlon, m, s);
    s *= r;
  }
}

// Block b -> (ring row, channel tile): the tiles of a row are kXcds blocks apart, so one XCD's L2 serves the whole
// [nlon, C] slab of a ring once.  false: a block past the last row (the grid is rounded up to kXcds rows).
__device__ __forceinline__ bool block_ring(int64_t rows, int ctiles, int64_t &row, int &ct) {
  const int64_t blk = blockIdx.x, t = blk / kXcds;
  ct = (int)(t % ctiles);
  row = (t / ctiles) * kXcds + blk % kXcds;
  return row < rows;
}

inline int64_t grid_blocks(int64_t rows, int ctiles) { return (rows + kXcds - 1) / kXcds * kXcds * ctiles; }

// ---- what a ring's block does around its transform: the regular grid's kernels and the reduced grid's share these ----
// xp, out, gp and xo point at channel c0 of the ring's first longitude (of its column of order 0); tw is the ring's own
// nlon-entry table.  A ring carries the orders m <= M (the regular grid: M = lmax).

// The ring into LDS: z[k] = x[2k] + i x[2k + 1] (half) or x[k] + 0 i.
template <typename TIn>
__device__ __forceinline__ void load_ring(cpx *__restrict__ sm, const TIn *__restrict__ xp, int nlon, int C, int c0,
                                          const Plan &pl) {
  const int tmask = pl.tile - 1;
  const int nx = nlon << pl.tile_log2;
  // lanes run over (longitude, channel), the channel fastest: a longitude moves one contiguous segment
#pragma unroll 4
  for (int e = threadIdx.x; e < nx; e += kThreads) {
    const int cc = e & tmask, i = e >> pl.tile_log2;
    const double v = c0 + cc < C ? (double)xp[(int64_t)i * C + cc] : 0.0;
    if (pl.half) {
      reinterpret_cast<double *>(sm + cc * pl.pitch + slot(i >> 1))[i & 1] = v;
    } else {
      sm[cc * pl.pitch + slot(i)] = cpx{v, 0.0 * v};          // 0 v: a NaN fills both components
    }
  }
  __syncthreads();
}

// The transformed ring to the workspace: out[+-m] = (cos, sin) sums of order m <= M, zeros for M < m <= L.
__device__ __forceinline__ void store_orders(const cpx *__restrict__ sm, const cpx *__restrict__ tw,
                                             double *__restrict__ out, int L, int M, int C, int c0, const Plan &pl) {
  const int tmask = pl.tile - 1;
  const int no = (L + 1) << pl.tile_log2;
  for (int e = threadIdx.x; e < no; e += kThreads) {
    const int cc = e & tmask, m = e >> pl.tile_log2;
    if (c0 + cc >= C) continue;
    if (m > M) {                                              // an order the ring does not carry (m >= 1)
      out[(int64_t)m * C + cc] = 0.0;
      out[-(int64_t)m * C + cc] = 0.0;
      continue;
    }
    const cpx *z = sm + cc * pl.pitch;
    cpx X = z[slot(m)];
    if (pl.half) {
      // X_m = E_m + w^m O_m, E = (Z_m + conj Z_{n-m}) / 2, O = (Z_m - conj Z_{n-m}) / 2i, w = exp(-2 pi i / nlon)
      const cpx zn = z[slot(m ? pl.n - m : 0)], w = tw[m];
      const cpx E = {0.5 * (X.x + zn.x), 0.5 * (X.y - zn.y)}, O = {0.5 * (X.y + zn.y), -0.5 * (X.x - zn.x)};
      X = cadd(E, cmul(O, w.x, -w.y));
    }
    out[(int64_t)m * C + cc] = X.x;
    if (m > 0) out[-(int64_t)m * C + cc] = -X.y;
  }
}

// The spectrum of the real ring into LDS, from the workspace columns of the orders m <= M: Xt_0 = cos_0, Xt_m = (cos_m -
// i sin_m) / 2 for 1 <= m <= M, Xt_{nlon-m} = conj Xt_m, the rest (the Nyquist order included) zero.
__device__ __forceinline__ void load_orders(cpx *__restrict__ sm, const cpx *__restrict__ tw,
                                            const double *__restrict__ gp, int M, int C, int c0, const Plan &pl) {
  const int tmask = pl.tile - 1;
  const int ni = pl.n << pl.tile_log2;
  for (int e = threadIdx.x; e < ni; e += kThreads) {
    const int cc = e & tmask, m = e >> pl.tile_log2;
    const bool live = c0 + cc < C;
    cpx v = {0.0, 0.0};
    if (pl.half) {
      // z_k = x_2k + i x_2k+1 = sum_m [(A + B) + i w^m (A - B)] w_n^(k m), A = Xt_m, B = conj Xt_{n-m}, w = exp(2 pi i / nlon)
      cpx A = {0.0, 0.0}, B = {0.0, 0.0};
      if (live && m <= M) {
        A.x = gp[(int64_t)m * C + cc];
        if (m > 0) A = cpx{0.5 * A.x, -0.5 * gp[-(int64_t)m * C + cc]};
      }
      const int k = pl.n - m;
      if (live && m > 0 && k <= M) B = cpx{0.5 * gp[(int64_t)k * C + cc], 0.5 * gp[-(int64_t)k * C + cc]};
      const cpx w = tw[m];
      const cpx t = cmul(csub(A, B), w.x, w.y);
      v = cpx{A.x + B.x - t.y, A.y + B.y + t.x};
    } else if (live && m <= M) {
      // x = Re sum_m (cos_m - i sin_m) w^(m i); 0 times the other component: a NaN fills both
      const double gc = gp[(int64_t)m * C + cc], gs = m > 0 ? gp[-(int64_t)m * C + cc] : 0.0;
      v = cpx{gc + 0.0 * gs, 0.0 * gc - gs};
    }
    sm[cc * pl.pitch + slot(m)] = v;
  }
  __syncthreads();
}

// The ring out of LDS, times the latitude's weight w.
template <typename TOut>
__device__ __forceinline__ void store_ring(const cpx *__restrict__ sm, TOut *__restrict__ xo, double w, int nlon, int C,
                                           int c0, const Plan &pl) {
  const int tmask = pl.tile - 1;
  const int nx = nlon << pl.tile_log2;
#pragma unroll 4
  for (int e = threadIdx.x; e < nx; e += kThreads) {
    const int cc = e & tmask, i = e >> pl.tile_log2;
    if (c0 + cc >= C) continue;
    const double v = pl.half ? reinterpret_cast<const double *>(sm + cc * pl.pitch + slot(i >> 1))[i & 1]
                             : sm[cc * pl.pitch + slot(i)].x;
    xo[(int64_t)i * C + cc] = (TOut)(v * w);
  }
}

// ring[row, lmax +- m, c] = sum_i x[row, i, c] (cos, sin)(2 pi m i / nlon), m <= lmax
template <typename TIn>
__global__ __launch_bounds__(kThreads) void k_sht_lon_fft_fwd(const TIn *__restrict__ x, const cpx *__restrict__ tw,
                                                              double *__restrict__ ring, int64_t rows, int nlon, int L,
                                                              int C, int ctiles, const Plan pl) {
  extern __shared__ cpx fft_sm[];
  cpx *sm = fft_sm;
  int64_t row;
  int ct;
  if (!block_ring(rows, ctiles, row, ct)) return;
  const int c0 = ct << pl.tile_log2;
  load_ring(sm, x + row * (int64_t)nlon * C + c0, nlon, C, c0, pl);
  transform<-1>(sm, tw, pl, nlon);
  store_orders(sm, tw, ring + (row * (int64_t)(2 * L + 1) + L) * C + c0, L, L, C, c0, pl);
}

// x[row, i, c] = lat_w sum_{m <= lmax} ring[row, lmax + m, c] cos(2 pi m i / nlon) + ring[row, lmax - m, c] sin(...)
template <typename TOut>
__global__ __launch_bounds__(kThreads) void k_sht_lon_fft_inv(const double *__restrict__ ring, const cpx *__restrict__ tw,
                                                              const double *__restrict__ lat_w, TOut *__restrict__ x,
                                                              int64_t rows, int nlat, int nlon, int L, int C, int ctiles,
                                                              const Plan pl) {
  extern __shared__ cpx fft_sm[];
  cpx *sm = fft_sm;
  int64_t row;
  int ct;
  if (!block_ring(rows, ctiles, row, ct)) return;
  const int c0 = ct << pl.tile_log2;
  load_orders(sm, tw, ring + (row * (int64_t)(2 * L + 1) + L) * C + c0, L, C, c0, pl);
  transform<1>(sm, tw, pl, nlon);
  const double w = lat_w ? lat_w[row % nlat] : 1.0;
  store_ring(sm, x + row * (int64_t)nlon * C + c0, w, nlon, C, c0, pl);
}

// ---- reduced grids: a ring length of its own on every latitude (gwen_sht_rings_fft_transform) -------------------------
// Ring j of ring_nlon[j] longitudes is a mixed ring where ring_nlon[j] = 2^a 3^b 5^c -- the transform above on the ring's
// own slice of the ring-by-ring twiddle table -- and a Bluestein ring otherwise: with n = nlon / 2 (even nlon, the same
// real-to-half-complex trick and split step) or n = nlon, c_k = exp(-i pi k^2 / n) and j k = (j^2 + k^2 - (k - j)^2) / 2,
//
//   Z_k = sum_j z_j exp(-2 pi i j k / n) = c_k sum_j (z_j c_j) conj(c_{k-j}),
//
// a cyclic convolution of length M = 2^a 3^b 5^c >= 2 n - 1 of a = (z c, zeros) with h_k = conj(c_k), |k| < n:
// transform<-1>, times H = FFT_M(h) / M, transform<+1>, on the plan {n = M, half = 0} and the M-entry table of M.  The
// inverse DFT is the same with conj(c) and conj(H) (h is even, so FFT_M(conj h) = conj FFT_M(h)).  A block owns one ring
// of one item and a tile of channels, the tile by tile_log2_of() of the ring's points in LDS (n, or M); the grid has the
// tile count of the longest ring on every ring, and the blocks that a shorter ring does not need return at once.

constexpr int kRingMixed = 1, kRingBluestein = 2;

// one record a ring, made on the host once; offsets in complex entries
struct __attribute__((aligned(16))) RingPlan {
  int kind;                            // kRingMixed or kRingBluestein
  int n;                               // the complex FFT of the ring: nlon / 2 (even nlon) or nlon
  int M;                               // Bluestein: the length of the convolution; mixed: 0
  int chirp, filter, tw;               // Bluestein: where c [n], H [M] and the table of M [M] start in their arrays
  int pad[2];
};

struct RingTables {
  const RingPlan *plan;                // [nlat]
  const cpx *chirp, *filter, *tw;
};

// The ring of the b-th row of blocks: from the equator outwards, nlat / 2, nlat / 2 - 1, nlat / 2 + 1, ...  On a reduced
// Gaussian grid that is the longest rings first, so the short polar rings fill the tail of the launch.
__device__ __forceinline__ int ring_of(int b, int nlat) {
  const int h = nlat >> 1;
  return b & 1 ? h - ((b + 1) >> 1) : h + (b >> 1);
}

// The LDS slots of a block bound from above, over every ring of at most max_points points in LDS (n or M) at C channels:
// a tile of t channels holds rings of at most kPoints / t points.
inline int ring_lds_slots(int max_points, int C) {
  int most = 0;
  for (int lg = tile_log2_of(1, C); lg >= 0; --lg) {
    const int len = max_points < (kPoints >> lg) ? max_points : kPoints >> lg;
    const int slots = (slot(len - 1) + 1) << lg;
    if (slots > most) most = slots;
  }
  return most;
}

// The plans of a block's ring into LDS -- plans[0] the ring's (what the loads, the split step and a mixed ring's transform
// read), plans[1] the convolution's of a Bluestein ring -- and a barrier.  false, before the barrier and for the whole
// block: the ring has no channel tile ct, or its record is not one this launch has the LDS for.
__device__ __forceinline__ bool ring_plans(const RingPlan &rp, int nlon, int C, int ct, int lds_slots, Plan *plans) {
  const int half = nlon % 2 == 0, n = half ? nlon / 2 : nlon;
  if ((rp.kind != kRingMixed && rp.kind != kRingBluestein) || rp.n != n) return false;
  const int len = rp.kind == kRingBluestein ? rp.M : n;
  if (len < n || len > kPoints) return false;
  const int lg = tile_log2_of(len, C), pitch = slot(len - 1) + 1;
  if ((ct << lg) >= C || (pitch << lg) > lds_slots) return false;
  if (threadIdx.x == 0) {
    for (int i = 0; i < 2; ++i) {
      Plan &p = plans[i];
      p.n = i ? len : n;
      p.half = i ? 0 : half;
      p.tile = 1 << lg;
      p.tile_log2 = lg;
      p.pitch = pitch;
      set_stages(p, i ? len : rp.kind == kRingMixed ? n : 1);
    }
  }
  __syncthreads();
  return true;
}

// a_k *= t_k (SGN = -1) or conj t_k (SGN = +1) for k < count; zeros from there to `upto`.  Never skipped: a NaN of one
// component reaches both.
template <int SGN>
__device__ __forceinline__ void times_table(cpx *__restrict__ sm, const cpx *__restrict__ t, int count, int upto,
                                            const Plan &pl) {
  const int tmask = pl.tile - 1;
  const int total = upto << pl.tile_log2;
  for (int e = threadIdx.x; e < total; e += kThreads) {
    const int cc = e & tmask, k = e >> pl.tile_log2;
    cpx *p = sm + cc * pl.pitch + slot(k);
    if (k < count) {
      const cpx w = t[k];
      *p = cmul(*p, w.x, -(double)SGN * w.y);
    } else {
      *p = cpx{0.0, 0.0};
    }
  }
  __syncthreads();
}

// The n-point DFT of sign SGN of every channel's z[0 .. n), in place, as the convolution above.
template <int SGN>
__device__ __forceinline__ void bluestein(cpx *__restrict__ sm, const RingTables &tb, const RingPlan &rp, const Plan &pl,
                                          const Plan &conv) {
  const cpx *chirp = tb.chirp + rp.chirp, *tw = tb.tw + rp.tw;
  times_table<SGN>(sm, chirp, pl.n, conv.n, conv);
  transform<-1>(sm, tw, conv, conv.n);
  times_table<SGN>(sm, tb.filter + rp.filter, conv.n, conv.n, conv);
  transform<1>(sm, tw, conv, conv.n);
  times_table<SGN>(sm, chirp, pl.n, pl.n, conv);
}

// Block -> (ring, item, channel tile) by block_ring() over the rows (ring order from the equator, item).
__device__ __forceinline__ bool block_ragged_ring(int64_t rows, int ctiles, int nlat, int nb, int &j, int64_t &item,
                                                  int &ct) {
  int64_t row;
  if (!block_ring(rows, ctiles, row, ct)) return false;
  j = ring_of((int)(row / nb), nlat);
  item = row % nb;
  return true;
}

// ring[item, j, lmax +- m, c] = sum_i x[item, ring_start[j] + i, c] (cos, sin)(2 pi m i / ring_nlon[j]) for m <= M_j =
// min(lmax, (ring_nlon[j] - 1) / 2), zeros for M_j < m <= lmax; tw is one table a ring, end to end
template <typename TIn>
__global__ __launch_bounds__(kThreads) void k_sht_rings_lon_fft_fwd(
    const TIn *__restrict__ x, const cpx *__restrict__ tw, const int *__restrict__ ring_nlon,
    const int64_t *__restrict__ ring_start, const RingTables tb, double *__restrict__ ring, int64_t rows, int64_t P,
    int nlat, int nb, int L, int C, int ctiles, int lds_slots) {
  extern __shared__ cpx fft_sm[];
  __shared__ Plan plans[2];
  cpx *sm = fft_sm;
  int j, ct;
  int64_t item;
  if (!block_ragged_ring(rows, ctiles, nlat, nb, j, item, ct)) return;
  const int nlon = ring_nlon[j];
  const RingPlan rp = tb.plan[j];
  if (!ring_plans(rp, nlon, C, ct, lds_slots, plans)) return;
  const Plan &pl = plans[0];
  const int c0 = ct << pl.tile_log2;
  const int M = L < ((nlon - 1) >> 1) ? L : (nlon - 1) >> 1;
  const int64_t start = ring_start[j];
  load_ring(sm, x + (item * P + start) * C + c0, nlon, C, c0, pl);
  if (rp.kind == kRingMixed) transform<-1>(sm, tw + start, pl, nlon);
  else bluestein<-1>(sm, tb, rp, pl, plans[1]);
  store_orders(sm, tw + start, ring + ((item * nlat + j) * (int64_t)(2 * L + 1) + L) * C + c0, L, M, C, c0, pl);
}

// x[item, ring_start[j] + i, c] = lat_w[j] sum_{m <= M_j} ring[item, j, lmax + m, c] cos(2 pi m i / ring_nlon[j]) +
// ring[item, j, lmax - m, c] sin(...); the columns above M_j are not read
template <typename TOut>
__global__ __launch_bounds__(kThreads) void k_sht_rings_lon_fft_inv(
    const double *__restrict__ ring, const cpx *__restrict__ tw, const int *__restrict__ ring_nlon,
    const int64_t *__restrict__ ring_start, const RingTables tb, const double *__restrict__ lat_w,
    TOut *__restrict__ x, int64_t rows, int64_t P, int nlat, int nb, int L, int C, int ctiles, int lds_slots) {
  extern __shared__ cpx fft_sm[];
  __shared__ Plan plans[2];
  cpx *sm = fft_sm;
  int j, ct;
  int64_t item;
  if (!block_ragged_ring(rows, ctiles, nlat, nb, j, item, ct)) return;
  const int nlon = ring_nlon[j];
  const RingPlan rp = tb.plan[j];
  if (!ring_plans(rp, nlon, C, ct, lds_slots, plans)) return;
  const Plan &pl = plans[0];
  const int c0 = ct << pl.tile_log2;
  const int M = L < ((nlon - 1) >> 1) ? L : (nlon - 1) >> 1;
  const int64_t start = ring_start[j];
  load_orders(sm, tw + start, ring + ((item * nlat + j) * (int64_t)(2 * L + 1) + L) * C + c0, M, C, c0, pl);
  if (rp.kind == kRingMixed) transform<1>(sm, tw + start, pl, nlon);
  else bluestein<1>(sm, tb, rp, pl, plans[1]);
  store_ring(sm, x + (item * P + start) * C + c0, lat_w ? lat_w[j] : 1.0, nlon, C, c0, pl);
}

}  // namespace sht_fft
