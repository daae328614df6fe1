// Static fields and forcings of the forecaster (include/gwen_hip.h, "Forcings"):
//     out[r, :] = x[r, :] + base[r % N, :] + sum_k f[r % N, k] wf[:, k]
// with f = [solar forcings at the clock's time (5), given columns (Fg)] of grid point r % N.  The clock {t, dt} is read
// from device memory: a captured step sees the current time on every replay, and gwen_forcing_advance moves it in
// stream order.  The solar vector is evaluated in fp64 (integer floor modulus of t first: t does not fit a float) and
// rounded once to fp32; it never reaches memory in the fused launch.
// Three launchers: the solar vector alone ([N, 5]), the fused embedding, the clock advance.  Fixed-order arithmetic,
// no atomics.
#include "common.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64, kRows = 8;
constexpr int64_t kYear = 31556926, kDay = 86400;
constexpr double kTwoPi = 6.283185307179586476925287, kPi = 3.141592653589793238462643;

// what the solar vector takes from the time alone
struct SolarTime {
  double sin_d, cos_d, e0, tau, h0, sin_g, cos_g;      // declination, eccentricity, tau, tau + E - pi, year phase
};

__device__ inline int64_t floor_mod(int64_t t, int64_t m) {
  const int64_t r = t % m;
  return r < 0 ? r + m : r;
}

// Spencer's series for the declination, the equation of time and the eccentricity factor
__device__ inline SolarTime solar_time(int64_t t) {
  const double g = kTwoPi * (double)floor_mod(t, kYear) / (double)kYear;
  const double tau = kTwoPi * (double)floor_mod(t, kDay) / (double)kDay;
  double s1, c1, s2, c2, s3, c3;
  sincos(g, &s1, &c1);
  sincos(2.0 * g, &s2, &c2);
  sincos(3.0 * g, &s3, &c3);
  const double d = 0.006918 - 0.399912 * c1 + 0.070257 * s1 - 0.006758 * c2 + 0.000907 * s2 - 0.002697 * c3 + 0.00148 * s3;
  const double E = 0.000075 + 0.001868 * c1 - 0.032077 * s1 - 0.014615 * c2 - 0.040849 * s2;
  SolarTime s;
  s.e0 = 1.000110 + 0.034221 * c1 + 0.001280 * s1 + 0.000719 * c2 + 0.000077 * s2;
  sincos(d, &s.sin_d, &s.cos_d);
  s.tau = tau;
  s.h0 = tau + E - kPi;
  s.sin_g = s1;
  s.cos_g = c1;
  return s;
}

// f = [e0 max(mu, 0), sin(tau + lon), cos(tau + lon), sin gamma, cos gamma]
__device__ inline void solar5(const SolarTime &s, double lat, double lon, float f[5]) {
  double sp, cp, sl, cl;
  sincos(lat, &sp, &cp);
  sincos(s.tau + lon, &sl, &cl);
  const double mu = sp * s.sin_d + cp * s.cos_d * cos(s.h0 + lon);
  f[0] = (float)(s.e0 * fmax(mu, 0.0));
  f[1] = (float)sl;
  f[2] = (float)cl;
  f[3] = (float)s.sin_g;
  f[4] = (float)s.cos_g;
}

__global__ __launch_bounds__(kThreads) void k_forcing_solar(const int64_t *__restrict__ clock,
                                                            const double *__restrict__ latlon, int64_t N,
                                                            float *__restrict__ out) {
  const SolarTime s = solar_time(clock[0]);
  for (int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x; n < N; n += (int64_t)gridDim.x * kThreads) {
    float f[5];
    solar5(s, latlon[2 * n], latlon[2 * n + 1], f);
#pragma unroll
    for (int k = 0; k < 5; ++k) out[5 * n + k] = f[k];
  }
}

// wave-scope LDS hand-over between lanes of one wave (release, wave barrier, acquire)
__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The embedding.  Block (bx, by): 4 waves, columns [4 LW by, 4 LW by + 4 LW) of every row, one float4 per lane: LW
// lanes span a row and a wave spans RP = 64 / LW consecutive rows, so that a wave's access is one contiguous KiB when
// H = 4 LW.  wf of those columns is transposed into LDS (wt[k][h]).  A wave takes G = 8 RP grid points at a time: lane l
// evaluates the solar vector of point l, the given columns are copied beside it (fw[point][k]); then every lane
// accumulates t[j] = sum_k f[point_j][k] wf[:, k] for its 8 points (fmaf from zero in increasing k; f a broadcast
// read), adds base -- once per POINT -- and streams the members: out = x + t.  Nothing but x and out scales with the
// members.  FP: capacity of the LDS arrays in forcing columns (F <= FP).
template <int LW, int FP>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(FP == 8 ? 4 : 2))) void k_forcing_embed(const int64_t *__restrict__ clock,
                                                            const double *__restrict__ latlon,
                                                            const float *__restrict__ given, int32_t Fg,
                                                            const float *__restrict__ wf,
                                                            const float *__restrict__ base, int64_t members, int64_t N,
                                                            const float *x, int32_t H, float *out) {
  constexpr int RP = 64 / LW, G = kRows * RP, FS = FP + 4, CW = 4 * LW;     // (FS: rows of fw on distinct banks)
  __shared__ __attribute__((aligned(16))) float wt[FP * CW];
  __shared__ __attribute__((aligned(16))) float fs[kWaves][G * FS];
  __shared__ SolarTime st;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int so = clock ? 5 : 0, F = so + Fg;
  const int64_t h0 = (int64_t)blockIdx.y * CW;
  for (int i = tid; i < CW * F; i += kThreads) {
    const int hl = i / F, k = i % F;
    wt[k * CW + hl] = h0 + hl < H ? wf[(h0 + hl) * F + k] : 0.0f;
  }
  if (clock && wave == 0) {
    const SolarTime s = solar_time(clock[0]);
    if (lane == 0) st = s;
  }
  __syncthreads();
  const int sub = lane / LW, cl = lane % LW;
  const int64_t col = h0 + 4 * cl;
  const bool on = col < H;
  float *fw = fs[wave];
  const float *wl = wt + 4 * cl;
  for (int64_t n0 = ((int64_t)blockIdx.x * kWaves + wave) * G; n0 < N; n0 += (int64_t)gridDim.x * kWaves * G) {
    if (clock && lane < G && n0 + lane < N) {
      float f[5];
      solar5(st, latlon[2 * (n0 + lane)], latlon[2 * (n0 + lane) + 1], f);
#pragma unroll
      for (int k = 0; k < 5; ++k) fw[lane * FS + k] = f[k];
    }
    for (int i = lane; i < G * Fg; i += 64)              // the group's given rows are contiguous
      if (n0 * Fg + i < N * Fg) fw[(i / Fg) * FS + so + i % Fg] = given[n0 * Fg + i];
    wave_sync();
    float4_t t[kRows];
#pragma unroll
    for (int j = 0; j < kRows; ++j) t[j] = float4_t{0.0f, 0.0f, 0.0f, 0.0f};
    int k = 0;
#pragma unroll 1
    for (; k + 4 <= F; k += 4) {
      const float4_t w0 = *reinterpret_cast<const float4_t *>(wl + k * CW),
                     w1 = *reinterpret_cast<const float4_t *>(wl + (k + 1) * CW),
                     w2 = *reinterpret_cast<const float4_t *>(wl + (k + 2) * CW),
                     w3 = *reinterpret_cast<const float4_t *>(wl + (k + 3) * CW);
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        const float4_t f4 = *reinterpret_cast<const float4_t *>(fw + (j * RP + sub) * FS + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          t[j][e] = fmaf(f4[0], w0[e], t[j][e]);
          t[j][e] = fmaf(f4[1], w1[e], t[j][e]);
          t[j][e] = fmaf(f4[2], w2[e], t[j][e]);
          t[j][e] = fmaf(f4[3], w3[e], t[j][e]);
        }
      }
    }
#pragma unroll 1
    for (; k < F; ++k) {
      const float4_t w = *reinterpret_cast<const float4_t *>(wl + k * CW);
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        const float fv = fw[(j * RP + sub) * FS + k];
#pragma unroll
        for (int e = 0; e < 4; ++e) t[j][e] = fmaf(fv, w[e], t[j][e]);
      }
    }
    // the lane's float4 of its j-th point is j strides on from its first; its first jn points exist
    const int64_t left = N - n0 - sub, stride = (int64_t)RP * H, first = (n0 + sub) * H + col;
    const int jn = !on || left <= 0 ? 0 : left >= (int64_t)G ? kRows : (int)((left + RP - 1) / RP);
    if (base) {
      const float *bp = base + first;
#pragma unroll
      for (int j = 0; j < kRows; ++j)
        if (j < jn) t[j] = t[j] + *reinterpret_cast<const float4_t *>(bp + j * stride);
    }
    // a member's 8 rows are loaded before any is stored; a lane reads and writes only its own float4s, so out may be x
#pragma unroll 1
    for (int64_t m = 0; m < members; ++m) {
      const float *xp = x + m * N * H + first;
      float *op = out + m * N * H + first;
      float4_t xv[kRows];
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        xv[j] = float4_t{0.0f, 0.0f, 0.0f, 0.0f};
        if (j < jn) xv[j] = *reinterpret_cast<const float4_t *>(xp + j * stride);
      }
#pragma unroll
      for (int j = 0; j < kRows; ++j)
        if (j < jn) *reinterpret_cast<float4_t *>(op + j * stride) = xv[j] + t[j];
    }
    wave_sync();                                         // the next group's forcings overwrite this group's
  }
}

__global__ void k_forcing_advance(int64_t *clock, int64_t n) { clock[0] = clock[0] + n * clock[1]; }

int blocks_for(int64_t work, int64_t per_block) {
  const int64_t b = (work + per_block - 1) / per_block;
  return (int)(b < 2048 ? (b > 0 ? b : 1) : 2048);       // grid-stride beyond: 8 blocks of 256 per CU
}

template <int LW>
void launch_embed(dim3 grid, hipStream_t st, int F, const int64_t *clock, const double *latlon, const float *given,
                  int32_t Fg, const float *wf, const float *base, int64_t members, int64_t N, const float *x, int32_t H,
                  float *out) {
  if (F <= 8)
    k_forcing_embed<LW, 8><<<grid, kThreads, 0, st>>>(clock, latlon, given, Fg, wf, base, members, N, x, H, out);
  else
    k_forcing_embed<LW, 64><<<grid, kThreads, 0, st>>>(clock, latlon, given, Fg, wf, base, members, N, x, H, out);
}

}  // namespace

extern "C" int gwen_forcing_advance(int64_t *clock, int64_t n, gwen_stream_t stream) {
  if (!clock || !gwen_aligned(clock, 8)) return GWEN_EINVAL;
  k_forcing_advance<<<1, 1, 0, gwen_stream(stream)>>>(clock, n);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

extern "C" int gwen_forcing_solar_f32(const int64_t *clock, const double *latlon, int64_t N, float *out,
                                      gwen_stream_t stream) {
  if (!clock || !gwen_aligned(clock, 8) || N < 0) return GWEN_EINVAL;
  if (!latlon || !gwen_aligned(latlon, 8)) return GWEN_EINVAL;
  if (N > 0 && (!out || !gwen_aligned(out, 4))) return GWEN_EINVAL;
  if (N > INT64_MAX / 5) return GWEN_ERANGE;
  if (N == 0) return GWEN_OK;
  k_forcing_solar<<<blocks_for(N, kThreads), kThreads, 0, gwen_stream(stream)>>>(clock, latlon, N, out);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

extern "C" int gwen_forcing_embed_f32(const int64_t *clock, const double *latlon, const float *given, int64_t Fg,
                                      const float *wf, const float *base, int64_t rows, int64_t N, const float *x,
                                      int64_t H, float *out, gwen_stream_t stream) {
  if (clock && (!gwen_aligned(clock, 8) || !latlon || !gwen_aligned(latlon, 8))) return GWEN_EINVAL;
  if (Fg < 0 || Fg > 64 || (Fg > 0 && (!given || !gwen_aligned(given, 4)))) return GWEN_EINVAL;
  const int64_t F = (clock ? 5 : 0) + Fg;
  if (F < 1 || F > 64 || N < 1 || rows < 0 || rows % N != 0 || H < 4 || H % 4 != 0) return GWEN_EINVAL;
  if (!x || !wf || !out || !gwen_aligned(x, 16) || !gwen_aligned(out, 16) || !gwen_aligned(wf, 16)) return GWEN_EINVAL;
  if (base && !gwen_aligned(base, 16)) return GWEN_EINVAL;
  if (H > (1 << 30) || rows > INT64_MAX / H || N > INT64_MAX / 64) return GWEN_ERANGE;
  if (rows == 0) return GWEN_OK;
  const int LW = H >= 256 ? 64 : H > 64 ? 32 : H > 32 ? 16 : 8;          // lanes across a row (H = 128: 32, 64: 16)
  const int64_t ty = (H + 4 * LW - 1) / (4 * LW);
  if (ty > 65535) return GWEN_ERANGE;
  const dim3 grid((unsigned)blocks_for(N, (int64_t)kWaves * kRows * (64 / LW)), (unsigned)ty);
  hipStream_t st = gwen_stream(stream);
  const int64_t members = rows / N;
  const int32_t fg = (int32_t)Fg, h = (int32_t)H;
  switch (LW) {
    case 8: launch_embed<8>(grid, st, (int)F, clock, latlon, given, fg, wf, base, members, N, x, h, out); break;
    case 16: launch_embed<16>(grid, st, (int)F, clock, latlon, given, fg, wf, base, members, N, x, h, out); break;
    case 32: launch_embed<32>(grid, st, (int)F, clock, latlon, given, fg, wf, base, members, N, x, h, out); break;
    default: launch_embed<64>(grid, st, (int)F, clock, latlon, given, fg, wf, base, members, N, x, h, out); break;
  }
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}
