// Row LayerNorm, forward and backward -- the unfused route of "K6 with LayerNorm" (interact_rows.hip has the fused
// one), the LayerNorm half of the InteractionNet block's backward, and ops.layer_norm.
//
// BUILD-DEFINED like the block (the reference has no edge MLP and no normalisation: its only graph layer is GCNConv);
// semantics are torch.nn.LayerNorm(F)'s, restated in fp64 by the tests:
//     LN(m)_c = (m_c - mu) * rstd * gamma_c + beta_c,  mu = mean_c m_c,  var = mean_c (m_c - mu)^2  (biased),
//     rstd = 1 / sqrt(var + eps)
// The variance is formed from DEVIATIONS about the mean (a second sweep over the row's registers), never as
// E[m^2] - mu^2: rows 1000 + N(0,1) lose every digit of their variance that way in fp32.
//
// A row is held by G = min(64, pow2ceil(F / 4)) adjacent lanes of one wave, one 16-byte piece per lane and sweep
// (F / 4 lanes per row up to 256 channels; two or four pieces per lane from there to 1024); the row's sums are G-lane
// butterflies (every lane of the row ends with the same bits).  Bandwidth kernels: every array crosses HBM once.
//   forward            out[r] = (res ? res[r] : 0) + LN(x[r])                           one group per row
//   forward, by target the same, plus agg[d] = sum (or mean) of LN(x[r]) over rowptr[d] <= r < rowptr[d + 1] in
//                      stored order (the aggregate is of LN(x), not of out): one group per TARGET, as
//                      k_act_pair_seg (interact_bwd.hip) does for the hidden layer; targets without rows get 0
//   backward           with y^ = (m - mu) rstd recomputed from m in registers and gg = g * gamma:
//                      g_m = rstd (gg - mean(gg) - y^ mean(gg * y^)); grad_gamma = sum_rows g * y^, grad_beta = sum_rows g
//                      as PER-BLOCK partials [chunk][grad_gamma | grad_beta] (256 rows a block, rows and groups summed
//                      in a fixed order), finished by gwen_reduce_chunks_batched.  No atomics: two runs bitwise equal.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxF = 1024;
// (NV below: 16-byte pieces per lane -- 1 up to 256 channels, 2 or 4 from there to kMaxF = 4 x 64 x 4)
constexpr int kBwdRows = 256;        // rows per block of the backward (= per partial chunk)

inline int group_of(int64_t F4) {
  int g = 1;
  while (g < F4 && g < 64) g <<= 1;
  return g;
}

template <int G>
__device__ inline float group_sum(float s) {
#pragma unroll
  for (int o = G / 2; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  return s;
}

// mu and rstd of the row whose pieces q, q + G, .. (< F4) this lane holds in v (absent pieces: ignored)
template <int G, int NV>
__device__ inline void row_stats(const float4_t (&v)[NV], int q, int F4, float eps, float &mu, float &rstd) {
  const float inv = 1.0f / (float)(4 * F4);
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < NV; ++k)
    if (q + k * G < F4) s += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
  mu = group_sum<G>(s) * inv;
  float ss = 0.0f;
#pragma unroll
  for (int k = 0; k < NV; ++k)
    if (q + k * G < F4) {
      const float4_t d = v[k] - float4_t{mu, mu, mu, mu};
      ss += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
    }
  rstd = 1.0f / sqrtf(group_sum<G>(ss) * inv + eps);
}

// SEG = false: group i takes row i.  SEG = true: group i takes TARGET i and walks its rows in stored order.
template <int G, int NV, bool SEG>
__global__ __launch_bounds__(kThreads) void k_layer_norm(const float *x, const float *__restrict__ gamma,
                                                         const float *__restrict__ beta, float eps, const float *res,
                                                         float *out, int64_t n, int F4,
                                                         const int32_t *__restrict__ rowptr, float *__restrict__ agg,
                                                         int mean) {
  const int q = threadIdx.x % G;
  const int64_t i = (blockIdx.x * (int64_t)kThreads + threadIdx.x) / G;
  if (i >= n) return;                                            // (whole groups: G divides the wave)
  const int64_t F = (int64_t)F4 * 4;
  float4_t ga[NV], be[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k)
    if (q + k * G < F4) {
      ga[k] = *reinterpret_cast<const float4_t *>(gamma + 4 * (q + k * G));
      be[k] = *reinterpret_cast<const float4_t *>(beta + 4 * (q + k * G));
    }
  auto one_row = [&](int64_t r, float4_t (&y)[NV]) {
    float4_t v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (q + k * G < F4) v[k] = *reinterpret_cast<const float4_t *>(x + r * F + 4 * (q + k * G));
    float mu, rstd;
    row_stats<G, NV>(v, q, F4, eps, mu, rstd);
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (q + k * G < F4) {
        y[k] = (v[k] - float4_t{mu, mu, mu, mu}) * float4_t{rstd, rstd, rstd, rstd} * ga[k] + be[k];
        if (out) {
          float4_t o = y[k];
          if (res) o += *reinterpret_cast<const float4_t *>(res + r * F + 4 * (q + k * G));
          *reinterpret_cast<float4_t *>(out + r * F + 4 * (q + k * G)) = o;
        }
      }
  };
  if constexpr (!SEG) {
    float4_t y[NV];
    one_row(i, y);
  } else {
    const int32_t s0 = rowptr[i], s1 = rowptr[i + 1];
    float4_t acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = float4_t{0.f, 0.f, 0.f, 0.f};
    for (int32_t r = s0; r < s1; ++r) {
      float4_t y[NV];
      one_row(r, y);
#pragma unroll
      for (int k = 0; k < NV; ++k)
        if (q + k * G < F4) acc[k] += y[k];
    }
    const float inv = mean && s1 > s0 ? 1.0f / (float)(s1 - s0) : 1.0f;
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (q + k * G < F4) {
        if (mean && s1 > s0) acc[k] *= float4_t{inv, inv, inv, inv};
        *reinterpret_cast<float4_t *>(agg + i * F + 4 * (q + k * G)) = acc[k];
      }
  }
}

// block b takes rows [256 b, 256 b + 256): group j of its 256 / G groups rows j, j + 256 / G, ..; a lane's column sums
// stay in registers over its rows, then the groups are added in group order through LDS
template <int G, int NV>
__global__ __launch_bounds__(kThreads) void k_layer_norm_bwd(const float *__restrict__ x, const float *g,
                                                             const float *__restrict__ gamma, float eps, float *gx,
                                                             float *__restrict__ partial, int64_t rows, int F4) {
  constexpr int NG = kThreads / G;
  __shared__ float red[NG * 2 * 4 * G * NV];                            // NG x [grad_gamma | grad_beta], F <= 4 G NV
  const int q = threadIdx.x % G, grp = threadIdx.x / G;
  const int64_t F = (int64_t)F4 * 4;
  const int64_t r0 = (int64_t)blockIdx.x * kBwdRows;
  const int64_t r1 = r0 + kBwdRows < rows ? r0 + kBwdRows : rows;
  float4_t ga[NV], sg[NV], sb[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    sg[k] = sb[k] = float4_t{0.f, 0.f, 0.f, 0.f};
    if (q + k * G < F4) ga[k] = *reinterpret_cast<const float4_t *>(gamma + 4 * (q + k * G));
  }
  const float invF = 1.0f / (float)F;
  for (int64_t r = r0 + grp; r < r1; r += NG) {
    float4_t v[NV], gg[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (q + k * G < F4) {
        v[k] = *reinterpret_cast<const float4_t *>(x + r * F + 4 * (q + k * G));
        gg[k] = *reinterpret_cast<const float4_t *>(g + r * F + 4 * (q + k * G));
      }
    float mu, rstd;
    row_stats<G, NV>(v, q, F4, eps, mu, rstd);
    float c1 = 0.0f, c2 = 0.0f;
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (q + k * G < F4) {
        v[k] = (v[k] - float4_t{mu, mu, mu, mu}) * float4_t{rstd, rstd, rstd, rstd};      // y^
        sb[k] += gg[k];
        sg[k] += gg[k] * v[k];
        gg[k] = gg[k] * ga[k];
        c1 += (gg[k][0] + gg[k][1]) + (gg[k][2] + gg[k][3]);
        const float4_t p = gg[k] * v[k];
        c2 += (p[0] + p[1]) + (p[2] + p[3]);
      }
    c1 = group_sum<G>(c1) * invF;
    c2 = group_sum<G>(c2) * invF;
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (q + k * G < F4) {
        const float4_t o = (gg[k] - float4_t{c1, c1, c1, c1} - v[k] * float4_t{c2, c2, c2, c2}) *
                           float4_t{rstd, rstd, rstd, rstd};
        *reinterpret_cast<float4_t *>(gx + r * F + 4 * (q + k * G)) = o;
      }
  }
  if (!partial) return;
  float *mine = red + (int64_t)grp * 2 * F;
#pragma unroll
  for (int k = 0; k < NV; ++k)
    if (q + k * G < F4) {
      *reinterpret_cast<float4_t *>(mine + 4 * (q + k * G)) = sg[k];
      *reinterpret_cast<float4_t *>(mine + F + 4 * (q + k * G)) = sb[k];
    }
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * F; c += kThreads) {
    float s = 0.0f;
    for (int j = 0; j < NG; ++j) s += red[(int64_t)j * 2 * F + c];
    partial[(int64_t)blockIdx.x * 2 * F + c] = s;
  }
}

inline bool ln_shape_ok(int64_t rows, int64_t F) {
  return rows >= 0 && F > 0 && F % 4 == 0 && F <= kMaxF && rows < (int64_t(1) << 31);
}

}  // namespace

extern "C" int gwen_layer_norm_supported(int64_t F) { return F > 0 && F % 4 == 0 && F <= kMaxF ? 1 : 0; }

extern "C" int gwen_layer_norm_f32(const float *x, const float *gamma, const float *beta, float eps, const float *res,
                                   float *out, int64_t rows, int64_t F, const int32_t *rowptr, float *agg,
                                   int64_t N_agg, int mean, gwen_stream_t stream) {
  if (!ln_shape_ok(rows, F) || N_agg < 0 || N_agg >= (int64_t(1) << 31) || !(eps >= 0.0f)) return GWEN_EINVAL;
  if (agg ? !rowptr : !out) return rows == 0 && !agg ? GWEN_OK : GWEN_EINVAL;
  const int64_t n = agg ? N_agg : rows;
  if (n == 0) return GWEN_OK;
  if (!gamma || !beta || (rows > 0 && !x)) return GWEN_EINVAL;
  if (out && (out == gamma || out == beta)) return GWEN_EINVAL;              // out may alias x / res row for row
  const void *al[] = {x, gamma, beta, res, out, agg};
  for (const void *p : al)
    if (p && !gwen_aligned(p, 16)) return GWEN_EINVAL;
  const int F4 = (int)(F / 4), G = group_of(F4);
  const int64_t blocks = (n * G + kThreads - 1) / kThreads;
  if (blocks >= (int64_t(1) << 31)) return GWEN_ERANGE;
  hipStream_t st = gwen_stream(stream);
  const int nv = (F4 + G - 1) / G;                                            // 1 below 64 lanes; 1 .. 4 at 64
#define GWEN_LN(GG, NV)                                                                                      \
  if (G == GG && (nv == NV || (nv == 3 && NV == 4))) {                                                       \
    if (agg) k_layer_norm<GG, NV, true><<<(unsigned)blocks, kThreads, 0, st>>>(x, gamma, beta, eps, res, out, n, F4, rowptr, agg, mean); \
    else k_layer_norm<GG, NV, false><<<(unsigned)blocks, kThreads, 0, st>>>(x, gamma, beta, eps, res, out, n, F4, nullptr, nullptr, 0);  \
  }
  GWEN_LN(1, 1) GWEN_LN(2, 1) GWEN_LN(4, 1) GWEN_LN(8, 1) GWEN_LN(16, 1) GWEN_LN(32, 1) GWEN_LN(64, 1) GWEN_LN(64, 2) GWEN_LN(64, 4)
#undef GWEN_LN
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

extern "C" int64_t gwen_layer_norm_bwd_chunks(int64_t rows) {
  return rows < 0 ? GWEN_EINVAL : (rows + kBwdRows - 1) / kBwdRows;
}

extern "C" int gwen_layer_norm_bwd_f32(const float *x, const float *g, const float *gamma, float eps, float *gx,
                                       float *partial, int64_t rows, int64_t F, gwen_stream_t stream) {
  if (!ln_shape_ok(rows, F) || !(eps >= 0.0f)) return GWEN_EINVAL;
  if (rows == 0) return GWEN_OK;
  if (!x || !g || !gamma || !gx || gx == x) return GWEN_EINVAL;              // gx may alias g row for row
  const void *al[] = {x, g, gamma, gx, partial};
  for (const void *p : al)
    if (p && !gwen_aligned(p, 16)) return GWEN_EINVAL;
  const int F4 = (int)(F / 4), G = group_of(F4);
  const int64_t blocks = gwen_layer_norm_bwd_chunks(rows);
  hipStream_t st = gwen_stream(stream);
  const int nv = (F4 + G - 1) / G;
#define GWEN_LN(GG, NV)                                     \
  if (G == GG && (nv == NV || (nv == 3 && NV == 4)))        \
    k_layer_norm_bwd<GG, NV><<<(unsigned)blocks, kThreads, 0, st>>>(x, g, gamma, eps, gx, partial, rows, F4);
  GWEN_LN(1, 1) GWEN_LN(2, 1) GWEN_LN(4, 1) GWEN_LN(8, 1) GWEN_LN(16, 1) GWEN_LN(32, 1) GWEN_LN(64, 1) GWEN_LN(64, 2) GWEN_LN(64, 4)
#undef GWEN_LN
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}
