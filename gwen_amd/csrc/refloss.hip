// The reference's ensemble losses (src/gwen/loss_functions.py: CRPSLoss, EnsembleVarRegLoss, MaskedLoss), one pass over
// the data per direction (include/gwen_hip.h has the formulas):
//   * Gaussian CRPS of pred [A, M, R] against target [A, R], per sample of S consecutive points;
//   * L1 minus alpha times the unbiased ensemble variance, value and gradient together;
//   * the masked mean of an element-wise L1 / squared error, value and gradient together.
// A point's members are R floats apart, so a wave reads 64 (256 on the 16-byte path) consecutive columns of every member
// plane.  Up to 32 members stay in registers between the sweeps (mean, then deviations about it, then the gradient);
// above that the later sweeps read the block's tile again.  mu, sigma, z and the cdf never leave registers.
// Every block owns the SAME kTile consecutive points on either path (4 bytes or 16 bytes per lane), leaves one value per
// point in LDS and sums them in point order, so the bits depend on neither the path nor the alignment; per-block partial
// sums go to the workspace and a second launch adds them in block order.  No atomics: two runs are bitwise equal.
// The member chain, the block sum, the bucket dispatch and the alignment check are csrc/members.h's.
#include "members.h"

namespace {

using namespace gwen::ens;

constexpr int kThreads = 256;
constexpr int kTile = 1024;                     // points (elements) of one block: 4 per thread
constexpr int64_t kMaxElems = int64_t(1) << 40;    // of a tensor
constexpr int64_t kMaxPoints = int64_t(1) << 33;   // of a launch: one block per kTile points
constexpr float kSqrt2 = 1.41421356237309504880f;
constexpr float kInvSqrtPi = 0.56418958354775628695f;

// MB > 0: at most MB members, held in registers (the chain of members.h); MB == 0: any number, a runtime loop
template <int MB, typename F>
__device__ __forceinline__ void for_members(int M, F &&f) {
  if constexpr (MB > 0) {
    members<0, MB>(M, f);
  } else {
    for (int i = 0; i < M; ++i) f(i);
  }
}

// sum += v with the rounding error carried in c (Kahan): a long sum in a fixed order keeps the error of one rounding,
// whatever the number of members or points (-fno-fast-math: the compiler leaves the expression alone)
__device__ __forceinline__ void kadd(float &sum, float &c, float v) {
  const float y = v - c;
  const float t = sum + y;
  c = (t - sum) - y;
  sum = t;
}

// the next member plane; up to MB members the address stays a vector one: no scalar base per member (they spill)
template <int MB, typename T>
__device__ __forceinline__ void bump(T *&p, int64_t R) {
  p += R;
  if constexpr (MB > 0) asm volatile("" : "+v"(p));
}

template <int VEC>
__device__ __forceinline__ void load_vec(const float *p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4_t q = *reinterpret_cast<const float4_t *>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = q[k];
  } else {
    v[0] = *p;
  }
}

template <int VEC>
__device__ __forceinline__ void store_vec(float *p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    float4_t q;
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = v[k];
    *reinterpret_cast<float4_t *>(p) = q;
  } else {
    *p = v[0];
  }
}

// the members of VEC consecutive points, R floats apart from pp on: registers up to MB, else read again
template <int MB, int VEC>
struct Members {
  float x[MB > 0 ? MB : 1][VEC];
  const float *pp;
  int64_t R;

  // first sweep: f(i, v) on the loaded values, which stay in x when MB > 0
  template <typename F>
  __device__ __forceinline__ void load(int M, F &&f) {
    const float *q = pp;
    for_members<MB>(M, [&](auto i_) {
      const int i = i_;
      float v[VEC];
      load_vec<VEC>(q, v);
      if constexpr (MB > 0) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) x[i][k] = v[k];
      }
      f(i, v);
      bump<MB>(q, R);
    });
  }

  // later sweeps
  template <typename F>
  __device__ __forceinline__ void each(int M, F &&f) {
    const float *q = pp;
    for_members<MB>(M, [&](auto i_) {
      const int i = i_;
      float v[VEC];
      if constexpr (MB > 0) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[k] = x[i][k];
      } else {
        load_vec<VEC>(q, v);
        q += R;
      }
      f(i, v);
    });
  }

  // mu = the mean, ss = the sum of squared deviations about mu (a second sweep: never E[x^2] - mu^2).  The mean is
  // taken of the differences to the first member, x_0 + sum (x_i - x_0) / M: exact for identical members (s == 0
  // exactly where the members are equal) and free of the offset's rounding when the members are close (csrc/products.hip)
  __device__ __forceinline__ void stats(int M, float (&mu)[VEC], float (&ss)[VEC]) {
    float sum[VEC], r0[VEC], c[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) sum[k] = r0[k] = c[k] = 0.0f;
    load(M, [&](int i, const float (&v)[VEC]) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        r0[k] = i == 0 ? v[k] : r0[k];
        kadd(sum[k], c[k], v[k] - r0[k]);
      }
    });
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      mu[k] = r0[k] + sum[k] / (float)M;
      ss[k] = c[k] = 0.0f;
    }
    each(M, [&](int, const float (&v)[VEC]) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const float d = v[k] - mu[k];
        kadd(ss[k], c[k], d * d);
      }
    });
  }
};

// Where a thread's points lie.  Block b owns the points [b kTile, b kTile + n); on the 16-byte path thread t takes
// 4 t .. 4 t + 3 in one trip, else t + 256 k in trip k.  A lane past the end reads the tile's first point again and its
// result is dropped (no load under a per-lane condition).
template <int VEC>
struct Trip {
  int local;
  bool valid;
  int64_t p;
  __device__ __forceinline__ Trip(int k, int64_t base, int n) {
    local = VEC == 4 ? 4 * (int)threadIdx.x : k * kThreads + (int)threadIdx.x;
    valid = local < n;
    p = base + (valid ? local : 0);
  }
};

// ---- Gaussian CRPS ----------------------------------------------------------------------------------------------------

struct Gauss {
  float s, sigma, z, q;
};
__device__ __forceinline__ Gauss gauss_point(float mu, float ss, float t, int M) {
  Gauss g;
  g.s = __builtin_sqrtf(ss / (float)(M - 1));
  g.sigma = g.s + 1e-6f;
  g.z = (t - mu) / (g.sigma * kSqrt2);
  g.q = 0.5f * erff(g.z);
  return g;
}

// Forward.  q^2 per point into LDS, then the sums of the samples the block touches: sample s0 = (b kTile) / S goes to
// ws[2 b] (the head), the last one -- if it is another -- to ws[2 b + 1] (the tail), and a sample that begins and ends
// inside the block is final: loss[s] = sum / S.  k_crps_finish_* add heads and tails of the blocks a sample spans.
template <int MB, int VEC>
__global__ __launch_bounds__(kThreads) void k_gauss_crps(const float *__restrict__ pred,
                                                         const float *__restrict__ target, int64_t A, int32_t M,
                                                         int64_t R, int64_t P, int64_t S, float *__restrict__ ws,
                                                         float *__restrict__ loss) {
  __shared__ __attribute__((aligned(16))) float q2[kTile];
  __shared__ float red[kThreads];
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kTile;
  const int n = P - base < kTile ? (int)(P - base) : kTile;
  for (int k = 0; k < 4 / VEC; ++k) {
    const Trip<VEC> tr(k, base, n);
    const int64_t a = A == 1 ? 0 : tr.p / R, r = tr.p - a * R;
    Members<MB, VEC> mem;
    mem.pp = pred + a * M * R + r;
    mem.R = R;
    float t[VEC], mu[VEC], ss[VEC];
    load_vec<VEC>(target + tr.p, t);
    mem.stats(M, mu, ss);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const float q = gauss_point(mu[j], ss[j], t[j], M).q;
      q2[tr.local + j] = tr.valid ? q * q : 0.0f;
    }
  }
  __syncthreads();
  const int64_t s0 = base / S;
  if (S >= kTile) {                             // at most two samples: [0, cut) and [cut, n)
    const int64_t c64 = (s0 + 1) * S - base;
    const int cut = c64 < n ? (int)c64 : n;
    const float4_t v = *reinterpret_cast<const float4_t *>(q2 + 4 * tid);
    float h = 0.0f, t = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool head = 4 * tid + j < cut;      // a select, never a product: a NaN stays in its own sample
      h += head ? v[j] : 0.0f;
      t += head ? 0.0f : v[j];
    }
    h = block_sum_all<kThreads>(h, &red);
    t = block_sum_all<kThreads>(t, &red);
    if (tid == 0) {
      ws[2 * (int64_t)blockIdx.x] = h;
      ws[2 * (int64_t)blockIdx.x + 1] = t;
    }
  } else {                                      // short samples: a thread per sample, points in order
    const int nseg = (int)((base + n - 1) / S - s0) + 1;
    for (int j = tid; j < nseg; j += kThreads) {
      const int64_t s = s0 + j;
      const int64_t lo64 = s * S - base, hi64 = lo64 + S;
      const int lo = lo64 < 0 ? 0 : (int)lo64, hi = hi64 > n ? n : (int)hi64;
      float acc = 0.0f, c = 0.0f;
      for (int i = lo; i < hi; ++i) kadd(acc, c, q2[i]);
      if (j == 0) ws[2 * (int64_t)blockIdx.x] = acc;
      else if (j == nseg - 1) ws[2 * (int64_t)blockIdx.x + 1] = acc;
      else loss[s] = acc / (float)S;
    }
  }
}

// block b's share of sample s, which it holds as its head or its tail
__device__ __forceinline__ float crps_partial(const float *__restrict__ ws, int64_t b, int64_t s, int64_t S) {
  return ws[2 * b + (s == (b * kTile) / S ? 0 : 1)];
}

// a thread per sample (short samples: a handful of blocks each), the blocks in order
__global__ __launch_bounds__(kThreads) void k_crps_finish_thread(const float *__restrict__ ws, int64_t NS, int64_t S,
                                                                 int64_t P, float *__restrict__ loss) {
  const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (s >= NS) return;
  const int64_t b0 = (s * S) / kTile, b1 = ((s + 1) * S - 1) / kTile;
  if (b0 == b1) {                               // inside one block: final already unless it is the block's head or tail
    const int64_t end = (b0 + 1) * kTile < P ? (b0 + 1) * kTile : P;
    if (s != (b0 * kTile) / S && s != (end - 1) / S) return;
  }
  float acc = 0.0f;
  for (int64_t b = b0; b <= b1; ++b) acc += crps_partial(ws, b, s, S);
  loss[s] = acc / (float)S;
}

// a block per sample (long samples: every block in between holds nothing else), strided then a tree
__global__ __launch_bounds__(kThreads) void k_crps_finish_block(const float *__restrict__ ws, int64_t S,
                                                                float *__restrict__ loss) {
  __shared__ float red[kThreads];
  const int64_t s = blockIdx.x;
  const int64_t b0 = (s * S) / kTile, b1 = ((s + 1) * S - 1) / kTile;
  float acc = 0.0f, c = 0.0f;
  for (int64_t b = b0 + threadIdx.x; b <= b1; b += kThreads) kadd(acc, c, crps_partial(ws, b, s, S));
  acc = block_sum_all<kThreads>(acc, &red);
  if (threadIdx.x == 0) loss[s] = acc / (float)S;
}

// Backward: the same sweeps, then grad x_i = a + b (x_i - mu) per point.
template <int MB, int VEC>
__global__ __launch_bounds__(kThreads) void k_gauss_crps_bwd(const float *__restrict__ gup,
                                                             const float *__restrict__ pred,
                                                             const float *__restrict__ target, int64_t A, int32_t M,
                                                             int64_t R, int64_t P, int64_t S,
                                                             float *__restrict__ grad_pred,
                                                             float *__restrict__ grad_target) {
  const int64_t base = (int64_t)blockIdx.x * kTile;
  const int n = P - base < kTile ? (int)(P - base) : kTile;
  const float invS = 1.0f / (float)S;
  for (int k = 0; k < 4 / VEC; ++k) {
    const Trip<VEC> tr(k, base, n);
    const int64_t a = A == 1 ? 0 : tr.p / R, r = tr.p - a * R;
    Members<MB, VEC> mem;
    mem.pp = pred + a * M * R + r;
    mem.R = R;
    float t[VEC], mu[VEC], ss[VEC], ga[VEC], gb[VEC], gt[VEC];
    load_vec<VEC>(target + tr.p, t);
    mem.stats(M, mu, ss);
    int64_t sk = tr.p / S, rk = tr.p - sk * S;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const Gauss g = gauss_point(mu[j], ss[j], t[j], M);
      const float c = gup[sk] * (2.0f * g.q * invS) * (expf(-g.z * g.z) * kInvSqrtPi);     // dL/dz
      gt[j] = c / (g.sigma * kSqrt2);
      ga[j] = -gt[j] / (float)M;
      // ds/dx_i = (x_i - mu) / ((M - 1) s), 0 where s == 0 (torch's std backward)
      gb[j] = g.s == 0.0f ? 0.0f : -c * (g.z / g.sigma) / ((float)(M - 1) * g.s);
      if (++rk == S) {
        rk = 0;
        ++sk;
      }
    }
    if (grad_pred) {                            // (uniform; only the stores are per lane)
      float *gp = grad_pred + a * M * R + r;
      mem.each(M, [&](int, const float (&v)[VEC]) {
        float o[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = ga[j] + gb[j] * (v[j] - mu[j]);
        if (tr.valid) store_vec<VEC>(gp, o);
        bump<MB>(gp, R);
      });
    }
    if (grad_target && tr.valid) store_vec<VEC>(grad_target + tr.p, gt);
  }
}

// ---- variance-regularised L1 ------------------------------------------------------------------------------------------

// target [A, M, R] (tm = M) or [A, 1, R] (tm = 1).  ws[2 b] = the block's sum of |x - t|, ws[2 b + 1] of the variances.
template <int MB, int VEC>
__global__ __launch_bounds__(kThreads) void k_varreg(const float *__restrict__ pred, const float *__restrict__ target,
                                                     int64_t A, int32_t M, int32_t tm, int64_t R, int64_t P,
                                                     float alpha, float *__restrict__ grad_pred,
                                                     float *__restrict__ grad_target, float *__restrict__ ws) {
  __shared__ __attribute__((aligned(16))) float l1s[kTile];
  __shared__ __attribute__((aligned(16))) float vars[kTile];
  __shared__ float red[kThreads];
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kTile;
  const int n = P - base < kTile ? (int)(P - base) : kTile;
  const float c_l1 = 1.0f / (float)(M * P);                              // 1 / numel
  const float c_var = alpha * 2.0f / ((float)(M - 1) * (float)P);        // M = 1: inf (NaN at alpha = 0), as torch
  const int64_t tstep = tm == 1 ? 0 : R;
  for (int k = 0; k < 4 / VEC; ++k) {
    const Trip<VEC> tr(k, base, n);
    const int64_t a = A == 1 ? 0 : tr.p / R, r = tr.p - a * R;
    Members<MB, VEC> mem;
    mem.pp = pred + a * M * R + r;
    mem.R = R;
    const float *tp = target + a * tm * R + r;
    float sum[VEC], r0[VEC], l1[VEC], sg[VEC], mu[VEC], ss[VEC], c0[VEC], c1[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) sum[j] = r0[j] = l1[j] = sg[j] = ss[j] = c0[j] = c1[j] = 0.0f;
    {
      const float *tq = tp;
      mem.load(M, [&](int i, const float (&v)[VEC]) {
        float t[VEC];
        load_vec<VEC>(tq, t);
        bump<MB>(tq, tstep);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const float d = v[j] - t[j];
          r0[j] = i == 0 ? v[j] : r0[j];
          kadd(sum[j], c0[j], v[j] - r0[j]);     // the mean from differences to the first member, as Members::stats
          kadd(l1[j], c1[j], __builtin_fabsf(d));
          sg[j] += sgnf(d);
        }
      });
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      mu[j] = r0[j] + sum[j] / (float)M;
      c0[j] = 0.0f;
    }
    {
      const float *tq = tp;
      float *gp = grad_pred ? grad_pred + a * M * R + r : nullptr;
      float *gt = (grad_target && tm != 1) ? grad_target + a * M * R + r : nullptr;
      mem.each(M, [&](int, const float (&v)[VEC]) {
        float t[VEC], o[VEC], ot[VEC];
        load_vec<VEC>(tq, t);                   // the target again: the tile is in cache
        bump<MB>(tq, tstep);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const float dev = v[j] - mu[j];
          kadd(ss[j], c0[j], dev * dev);
          const float sl = sgnf(v[j] - t[j]) * c_l1;
          o[j] = sl - c_var * dev;
          ot[j] = -sl;
        }
        if (gp) {
          if (tr.valid) store_vec<VEC>(gp, o);
          bump<MB>(gp, R);
        }
        if (gt) {
          if (tr.valid) store_vec<VEC>(gt, ot);
          bump<MB>(gt, R);
        }
      });
    }
    if (grad_target && tm == 1 && tr.valid) {
      float ot[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) ot[j] = -sg[j] * c_l1;
      store_vec<VEC>(grad_target + tr.p, ot);
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      l1s[tr.local + j] = tr.valid ? l1[j] : 0.0f;
      vars[tr.local + j] = tr.valid ? ss[j] / (float)(M - 1) : 0.0f;
    }
  }
  __syncthreads();
  const float4_t u = *reinterpret_cast<const float4_t *>(l1s + 4 * tid);
  const float4_t w = *reinterpret_cast<const float4_t *>(vars + 4 * tid);
  const float sl = block_sum_all<kThreads>(((u[0] + u[1]) + u[2]) + u[3], &red);
  const float sv = block_sum_all<kThreads>(((w[0] + w[1]) + w[2]) + w[3], &red);
  if (tid == 0) {
    ws[2 * (int64_t)blockIdx.x] = sl;
    ws[2 * (int64_t)blockIdx.x + 1] = sv;
  }
}

// loss = sum |x - t| / numel - alpha sum var / P over the blocks' partials: one block, strided then a tree
__global__ __launch_bounds__(kThreads) void k_varreg_final(const float *__restrict__ ws, int64_t nblocks, int32_t M,
                                                           int64_t P, float alpha, float *__restrict__ loss) {
  __shared__ float red[kThreads];
  float sl = 0.0f, sv = 0.0f, cl = 0.0f, cv = 0.0f;
  for (int64_t b = threadIdx.x; b < nblocks; b += kThreads) {
    kadd(sl, cl, ws[2 * b]);
    kadd(sv, cv, ws[2 * b + 1]);
  }
  sl = block_sum_all<kThreads>(sl, &red);
  sv = block_sum_all<kThreads>(sv, &red);
  if (threadIdx.x == 0) loss[0] = sl / (float)(M * P) + (-alpha * (sv / (float)P));
}

// ---- masked mean --------------------------------------------------------------------------------------------------------

constexpr int kMaskBlocks = 1024;

// part[b] = the sum of block b's share of the mask: groups of 4 consecutive values, strided over the grid
template <bool V4>
__global__ __launch_bounds__(kThreads) void k_mask_sum(const float *__restrict__ mask, int64_t n,
                                                       float *__restrict__ part) {
  __shared__ float red[kThreads];
  float acc = 0.0f, c = 0.0f;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; 4 * g < n; g += (int64_t)gridDim.x * kThreads) {
    if constexpr (V4) {                         // n % 4 == 0
      const float4_t v = *reinterpret_cast<const float4_t *>(mask + 4 * g);
      kadd(acc, c, ((v[0] + v[1]) + v[2]) + v[3]);
    } else {
      float v = 0.0f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {             // past the end: the last value again, dropped by a select
        const int64_t e = 4 * g + k;
        const float m = mask[e < n ? e : n - 1];
        v += e < n ? m : 0.0f;
      }
      kadd(acc, c, v);
    }
  }
  acc = block_sum_all<kThreads>(acc, &red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// ws[0] = the sum of the mask as given
__global__ __launch_bounds__(kThreads) void k_mask_total(float *__restrict__ ws, int32_t nparts) {
  __shared__ float red[kThreads];
  float acc = 0.0f;
  for (int i = threadIdx.x; i < nparts; i += kThreads) acc += ws[1 + i];
  acc = block_sum_all<kThreads>(acc, &red);
  if (threadIdx.x == 0) ws[0] = acc;
}

// KIND 0: |d|, 1: d^2.  ws[1 + kMaskBlocks + b] = the block's sum of l(out, target) mask.
template <int KIND, int VEC>
__global__ __launch_bounds__(kThreads) void k_masked_mean(const float *__restrict__ out,
                                                          const float *__restrict__ target,
                                                          const float *__restrict__ mask, int64_t total, int64_t inner,
                                                          int32_t mask_full, float *__restrict__ grad_out,
                                                          float *__restrict__ grad_target, float *__restrict__ ws) {
  __shared__ __attribute__((aligned(16))) float vals[kTile];
  __shared__ float red[kThreads];
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kTile;
  const int n = total - base < kTile ? (int)(total - base) : kTile;
  const float inv = 1.0f / ws[0];               // an all-zero mask: inf, and 0 * inf = NaN, as the expression
  for (int k = 0; k < 4 / VEC; ++k) {
    const Trip<VEC> tr(k, base, n);
    float o[VEC], t[VEC], m[VEC], g[VEC], gt[VEC];
    load_vec<VEC>(out + tr.p, o);
    load_vec<VEC>(target + tr.p, t);
    load_vec<VEC>(mask + (mask_full ? tr.p : tr.p % inner), m);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const float d = o[j] - t[j];
      const float l = KIND == 0 ? __builtin_fabsf(d) : d * d;
      const float dl = KIND == 0 ? sgnf(d) : 2.0f * d;
      vals[tr.local + j] = tr.valid ? l * m[j] : 0.0f;
      g[j] = dl * m[j] * inv;
      gt[j] = -g[j];
    }
    if (tr.valid) {
      if (grad_out) store_vec<VEC>(grad_out + tr.p, g);
      if (grad_target) store_vec<VEC>(grad_target + tr.p, gt);
    }
  }
  __syncthreads();
  const float4_t u = *reinterpret_cast<const float4_t *>(vals + 4 * tid);
  const float s = block_sum_all<kThreads>(((u[0] + u[1]) + u[2]) + u[3], &red);
  if (tid == 0) ws[1 + kMaskBlocks + (int64_t)blockIdx.x] = s;
}

__global__ __launch_bounds__(kThreads) void k_masked_final(const float *__restrict__ ws, int64_t nblocks,
                                                           float *__restrict__ loss) {
  __shared__ float red[kThreads];
  float acc = 0.0f, c = 0.0f;
  for (int64_t b = threadIdx.x; b < nblocks; b += kThreads) kadd(acc, c, ws[1 + kMaskBlocks + b]);
  acc = block_sum_all<kThreads>(acc, &red);
  if (threadIdx.x == 0) loss[0] = acc / ws[0];
}

// ---- launchers --------------------------------------------------------------------------------------------------------

// GWEN_OK when [A, M, R] is a shape the kernels address
int check_shape(int64_t A, int64_t M, int64_t R, int64_t min_m, int64_t max_m) {
  if (A < 1 || R < 1 || M < min_m || M > max_m) return GWEN_EINVAL;
  if (A > kMaxPoints || R > kMaxPoints / A || M > kMaxElems / (A * R)) return GWEN_ERANGE;
  return GWEN_OK;
}

int64_t tiles(int64_t points) { return (points + kTile - 1) / kTile; }

// f(MB, VEC) as integral constants for the member bucket (8, 32, or 0: more, the run-time loop) and the path
template <typename F>
int dispatch(int64_t M, bool vec4, F &&f) {
  return dispatch_bucket(gwen::ints<8, 32, 0>{}, M, [&](auto mb) {
    return vec4 ? f(mb, std::integral_constant<int, 4>()) : f(mb, std::integral_constant<int, 1>());
  });
}

int check_crps(int64_t A, int64_t M, int64_t R, int64_t S) {
  const int rc = check_shape(A, M, R, 2, 256);
  if (rc != GWEN_OK) return rc;
  return (S < 1 || R % S) ? GWEN_EINVAL : GWEN_OK;
}

}  // namespace

extern "C" int64_t gwen_gauss_crps_workspace_floats(int64_t A, int64_t M, int64_t R, int64_t S) {
  return check_crps(A, M, R, S) == GWEN_OK ? 2 * tiles(A * R) : 0;
}

extern "C" int gwen_gauss_crps_f32(const float *pred, const float *target, int64_t A, int64_t M, int64_t R, int64_t S,
                                   float *loss, float *workspace, int64_t workspace_floats, gwen_stream_t stream_) {
  const int rc = check_crps(A, M, R, S);
  if (rc != GWEN_OK) return rc;
  if (!pred || !target || !loss || !workspace || workspace_floats < gwen_gauss_crps_workspace_floats(A, M, R, S))
    return GWEN_EINVAL;
  if (!aligned_all({pred, target, loss, workspace}, 4)) return GWEN_EINVAL;
  const int64_t P = A * R, NS = P / S, nb = tiles(P);
  const bool vec4 = R % 4 == 0 && aligned_all({pred, target}, 16);
  hipStream_t st = gwen_stream(stream_);
  const int lrc = dispatch(M, vec4, [&](auto MB, auto VEC) {
    k_gauss_crps<decltype(MB)::value, decltype(VEC)::value>
        <<<(unsigned)nb, kThreads, 0, st>>>(pred, target, A, (int32_t)M, R, P, S, workspace, loss);
    GWEN_LAUNCH_CHECK();
    return (int)GWEN_OK;
  });
  if (lrc != GWEN_OK) return lrc;
  if (S < 4 * kTile)
    k_crps_finish_thread<<<(unsigned)((NS + kThreads - 1) / kThreads), kThreads, 0, st>>>(workspace, NS, S, P, loss);
  else
    k_crps_finish_block<<<(unsigned)NS, kThreads, 0, st>>>(workspace, S, loss);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

extern "C" int gwen_gauss_crps_bwd_f32(const float *grad_loss, const float *pred, const float *target, int64_t A,
                                       int64_t M, int64_t R, int64_t S, float *grad_pred, float *grad_target,
                                       gwen_stream_t stream_) {
  const int rc = check_crps(A, M, R, S);
  if (rc != GWEN_OK) return rc;
  if (!grad_loss || !pred || !target || (!grad_pred && !grad_target)) return GWEN_EINVAL;
  if (!aligned_all({grad_loss, pred, target, grad_pred, grad_target}, 4)) return GWEN_EINVAL;
  const int64_t P = A * R, nb = tiles(P);
  const bool vec4 = R % 4 == 0 && aligned_all({pred, target, grad_pred, grad_target}, 16);
  hipStream_t st = gwen_stream(stream_);
  return dispatch(M, vec4, [&](auto MB, auto VEC) {
    k_gauss_crps_bwd<decltype(MB)::value, decltype(VEC)::value>
        <<<(unsigned)nb, kThreads, 0, st>>>(grad_loss, pred, target, A, (int32_t)M, R, P, S, grad_pred, grad_target);
    GWEN_LAUNCH_CHECK();
    return (int)GWEN_OK;
  });
}

extern "C" int64_t gwen_varreg_l1_workspace_floats(int64_t A, int64_t M, int64_t R) {
  return check_shape(A, M, R, 1, INT32_MAX) == GWEN_OK ? 2 * tiles(A * R) : 0;
}

extern "C" int gwen_varreg_l1_f32(const float *pred, const float *target, int64_t A, int64_t M, int64_t R,
                                  int target_broadcast, float alpha, float *grad_pred, float *grad_target, float *loss,
                                  float *workspace, int64_t workspace_floats, gwen_stream_t stream_) {
  const int rc = check_shape(A, M, R, 1, INT32_MAX);
  if (rc != GWEN_OK) return rc;
  if (target_broadcast != 0 && target_broadcast != 1) return GWEN_EINVAL;
  if (!pred || !target || !loss || !workspace || workspace_floats < gwen_varreg_l1_workspace_floats(A, M, R))
    return GWEN_EINVAL;
  if (!aligned_all({pred, target, grad_pred, grad_target, loss, workspace}, 4)) return GWEN_EINVAL;
  const int64_t P = A * R, nb = tiles(P);
  const bool vec4 = R % 4 == 0 && aligned_all({pred, target, grad_pred, grad_target}, 16);
  const int32_t tm = target_broadcast ? 1 : (int32_t)M;
  hipStream_t st = gwen_stream(stream_);
  const int lrc = dispatch(M, vec4, [&](auto MB, auto VEC) {
    k_varreg<decltype(MB)::value, decltype(VEC)::value><<<(unsigned)nb, kThreads, 0, st>>>(
        pred, target, A, (int32_t)M, tm, R, P, alpha, grad_pred, grad_target, workspace);
    GWEN_LAUNCH_CHECK();
    return (int)GWEN_OK;
  });
  if (lrc != GWEN_OK) return lrc;
  k_varreg_final<<<1, kThreads, 0, st>>>(workspace, nb, (int32_t)M, P, alpha, loss);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

namespace {
int check_masked(int64_t outer, int64_t inner) {
  if (outer < 1 || inner < 1) return GWEN_EINVAL;
  if (outer > kMaxPoints || inner > kMaxPoints / outer) return GWEN_ERANGE;
  return GWEN_OK;
}
}  // namespace

extern "C" int64_t gwen_masked_mean_workspace_floats(int64_t outer, int64_t inner) {
  return check_masked(outer, inner) == GWEN_OK ? 1 + kMaskBlocks + tiles(outer * inner) : 0;
}

extern "C" int gwen_masked_mean_f32(const float *out, const float *target, const float *mask, int64_t outer,
                                    int64_t inner, int mask_full, int kind, float *grad_out, float *grad_target,
                                    float *loss, float *workspace, int64_t workspace_floats, gwen_stream_t stream_) {
  const int rc = check_masked(outer, inner);
  if (rc != GWEN_OK) return rc;
  if ((mask_full != 0 && mask_full != 1) || (kind != GWEN_MASKED_L1 && kind != GWEN_MASKED_MSE)) return GWEN_EINVAL;
  if (!out || !target || !mask || !loss || !workspace ||
      workspace_floats < gwen_masked_mean_workspace_floats(outer, inner))
    return GWEN_EINVAL;
  if (!aligned_all({out, target, mask, grad_out, grad_target, loss, workspace}, 4)) return GWEN_EINVAL;
  const int64_t total = outer * inner, nb = tiles(total), nmask = mask_full ? total : inner;
  // 16 bytes per lane: groups of 4 elements stay inside a row of the mask
  const bool vec4 = total % 4 == 0 && (mask_full || inner % 4 == 0) &&
                    aligned_all({out, target, mask, grad_out, grad_target}, 16);
  const bool mvec4 = nmask % 4 == 0 && gwen_aligned(mask, 16);
  int64_t mb = (nmask + 4 * kThreads - 1) / (4 * kThreads);
  mb = mb > kMaskBlocks ? kMaskBlocks : mb;
  hipStream_t st = gwen_stream(stream_);
  if (mvec4) k_mask_sum<true><<<(unsigned)mb, kThreads, 0, st>>>(mask, nmask, workspace + 1);
  else k_mask_sum<false><<<(unsigned)mb, kThreads, 0, st>>>(mask, nmask, workspace + 1);
  GWEN_LAUNCH_CHECK();
  k_mask_total<<<1, kThreads, 0, st>>>(workspace, (int32_t)mb);
  GWEN_LAUNCH_CHECK();
  auto pass = [&](auto KIND, auto VEC) {
    k_masked_mean<decltype(KIND)::value, decltype(VEC)::value><<<(unsigned)nb, kThreads, 0, st>>>(
        out, target, mask, total, inner, mask_full, grad_out, grad_target, workspace);
  };
  using std::integral_constant;
  if (kind == GWEN_MASKED_L1) {
    if (vec4) pass(integral_constant<int, 0>(), integral_constant<int, 4>());
    else pass(integral_constant<int, 0>(), integral_constant<int, 1>());
  } else {
    if (vec4) pass(integral_constant<int, 1>(), integral_constant<int, 4>());
    else pass(integral_constant<int, 1>(), integral_constant<int, 1>());
  }
  GWEN_LAUNCH_CHECK();
  k_masked_final<<<1, kThreads, 0, st>>>(workspace, nb, loss);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}
