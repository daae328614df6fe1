// Ensemble CRPS over the members axis, value, per-channel scores and gradient in one pass over pred [M, N, C]:
//     skill = (1/M) sum_i |x_i - y|,   pair = sum_i sum_j |x_i - x_j| = 2 sum_i c_i (x_i - r),
//     CRPS  = skill - k * pair,        c_i = #{j : x_j < x_i} - #{j : x_j > x_i}   (mid-rank form: ties share it)
// for any member r of the point (sum_i c_i = 0).  Differences to one member of the point are exact when the members
// are close (Sterbenz), so the pair term and the variance never cancel at large offsets.  c_i comes from O(M^2)
// counting up to 16 members and from a register bitonic network carrying member indices above (3.5 M^2 against
// ~5 M log2(M)^2 / 4 vector instructions per point: 3x fewer at 32 members, 4x at 64).
// Four launches, no atomics (bitwise reproducible): the weight sums, the pass (per-block per-channel partials), a
// fixed-order per-channel finish, and the scalar loss.
// The member chains, the network, the block sums, the pass geometry and the bucket dispatch are csrc/members.h's.
#include "members.h"

namespace {

using namespace gwen::ens;

constexpr int kThreads = 256;
constexpr int kMaxChunks = 2048;       // node chunks (blocks along N) of the pass: the partials' row count

// ws[0] = sum_n w_n (N without weights), ws[1] = sum_c v_c (C without weights); one block, fixed order
__global__ __launch_bounds__(1024) void k_ens_weight_sums(const float *__restrict__ node_w, int64_t N,
                                                          const float *__restrict__ chan_w, int64_t C,
                                                          float *__restrict__ ws) {
  __shared__ float part[2][1024];
  float a = 0.0f, b = 0.0f;
  if (node_w)
    for (int64_t i = threadIdx.x; i < N; i += 1024) a += node_w[i];
  if (chan_w)
    for (int64_t i = threadIdx.x; i < C; i += 1024) b += chan_w[i];
  block_sum<1024>(part, {a, b});
  if (threadIdx.x == 0) {
    ws[0] = node_w ? part[0][0] : (float)N;
    ws[1] = chan_w ? part[1][0] : (float)C;
  }
}

// sign(a - b) without a lane mask: a - b is 0 only when a == b (gradual underflow), and two scalings by 2^126 carry
// the smallest non-zero difference past 1 before the clamp
__device__ inline float sgn_diff(float a, float b) {
  return __builtin_amdgcn_fmed3f((a - b) * 0x1p126f * 0x1p126f, -1.0f, 1.0f);
}

// A validated call of the pass, as gwen_ens_crps_f32 names its arguments: what the dispatch hands to launch_pass.  The
// kernel itself keeps a parameter list: as one by-value struct the pointers lose __restrict__, and every instantiation
// compiles to other code (DESIGN, "One copy of each helper").
struct CrpsArgs {
  const float *pred, *target, *node_w, *chan_w;
  int64_t M, N, C;
  float pair_coef;
  float *grad_pred, *grad_target, *ws;
};

// The pass.  Thread (row, lc) of block (bx, by) owns VEC consecutive channels (vector column bx * CT + lc) and walks
// the nodes n = by * R + row, += gridDim.y * R: a wave reads 64 consecutive columns of every member plane (the planes
// are contiguous N*C runs).  MB: the member bucket (M <= MB); SORT: ranks from the bitonic network (VEC == 1), else by
// counting; GRAD: grad_pred written.  Per-thread partial sums of w*CRPS, w*(mean - y)^2 and w*s^2 per channel, reduced
// over the block's rows in LDS in a fixed order into ws[2 + C + (by * 3 + q) * C + c].
template <int MB, int VEC, bool SORT, bool GRAD>
__global__ __launch_bounds__(kThreads) void k_ens_crps(const float *__restrict__ pred, const float *__restrict__ target,
                                                       const float *__restrict__ node_w,
                                                       const float *__restrict__ chan_w, int32_t M_, int64_t N,
                                                       int32_t C, int32_t CT, int32_t R, float pair_coef,
                                                       float *__restrict__ grad_pred, float *__restrict__ grad_target,
                                                       float *__restrict__ ws) {
  static_assert(!SORT || VEC == 1, "the sorting network holds one point per thread");
  constexpr int kRed = 3 * VEC * kThreads;
  constexpr int kScatter = (SORT && GRAD) ? MB * kThreads : 0;
  __shared__ float lds[kRed > kScatter ? kRed : kScatter];
  const int tid = threadIdx.x;
  const int row = tid / CT, lc = tid - row * CT;
  const int Cv = VEC == 4 ? C / 4 : C;
  const int64_t col = (int64_t)blockIdx.x * CT + lc;
  const bool active = row < R && col < Cv;
  const int64_t plane_ = N * (int64_t)C;
  const float inv = 1.0f / (ws[0] * ws[1]);          // 1 / (sum w * sum v): 0 weights give inf, then NaN, as torch
  const float invM = 1.0f / (float)M_;
  const float varDiv = (float)(M_ - 1);               // M = 1: 0 / 0 = NaN, torch's unbiased variance of one value
  float acc[3][VEC];
  float vch[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    acc[0][v] = acc[1][v] = acc[2][v] = 0.0f;
    vch[v] = (active && chan_w) ? chan_w[col * VEC + v] : 1.0f;
  }
  if (active) {
    for (int64_t n = (int64_t)blockIdx.y * R + row; n < N; n += (int64_t)gridDim.y * R) {
      int M = M_;
      int64_t plane = plane_;
      fresh(M, plane);
      const int64_t off = n * C + col * VEC;
      const float wn = node_w ? node_w[n] : 1.0f;
      float x[MB][VEC], y[VEC];
      // the member loads: the POINTER passes the empty asm here, the offset in k_ens_products, whose loads must stay
      // global loads -- two bodies on purpose
      if constexpr (VEC == 4) {
        const float4_t t = *reinterpret_cast<const float4_t *>(target + off);
#pragma unroll
        for (int v = 0; v < 4; ++v) y[v] = t[v];
        const float *pp = pred + off;
        members<0, MB>(M, [&](auto I_) {
          constexpr int i = decltype(I_)::value;
          const float4_t p = *reinterpret_cast<const float4_t *>(pp);
#pragma unroll
          for (int v = 0; v < 4; ++v) x[i][v] = p[v];
          pp += plane;
          asm volatile("" : "+v"(pp));
        });
      } else {
        y[0] = target[off];
#pragma unroll
        for (int i = 0; i < MB; ++i) x[i][0] = __builtin_inff();      // pads sort behind every finite member
        const float *pp = pred + off;
        members<0, MB>(M, [&](auto I_) {
          constexpr int i = decltype(I_)::value;
          x[i][0] = *pp;
          pp += plane;
          asm volatile("" : "+v"(pp));
        });
      }
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const float yv = y[v], r = x[0][v];
        const float scale = wn * vch[v] * inv;
        float skill = 0.0f, sgn_sum = 0.0f, dsum = 0.0f, var = 0.0f, pair = 0.0f;
        // (dsum, dbar, var as in k_ens_products, but dsum shares the chain of skill and sgn_sum: two bodies)
        members<0, MB>(M, [&](auto I_) {
          constexpr int i = decltype(I_)::value;
          skill += __builtin_fabsf(x[i][v] - yv);
          sgn_sum += sgnf(x[i][v] - yv);
          dsum += x[i][v] - r;
        });
        const float dbar = dsum * invM;
        members<0, MB>(M, [&](auto I_) {
          constexpr int i = decltype(I_)::value;
          const float t = (x[i][v] - r) - dbar;
          var += t * t;
        });
        if constexpr (!SORT) {
          float cnt[MB];                       // integers, exact in fp32
#pragma unroll
          for (int i = 0; i < MB; ++i) cnt[i] = 0.0f;
          members<0, MB>(M, [&](auto I_) {
            constexpr int i = decltype(I_)::value;
            members<i + 1, MB>(M, [&](auto J_) {
              constexpr int j = decltype(J_)::value;
              const float s = sgn_diff(x[i][v], x[j][v]);
              cnt[i] += s;
              cnt[j] -= s;
            });
          });
          members<0, MB>(M, [&](auto I_) {
            constexpr int i = decltype(I_)::value;
            pair += cnt[i] * (x[i][v] - r);
          });
          if constexpr (GRAD) {
            members<0, MB>(M, [&](auto I_) {    // x[i][v] is not read again: it becomes the gradient
              constexpr int i = decltype(I_)::value;
              x[i][v] = scale * (sgnf(x[i][v] - yv) * invM - 2.0f * pair_coef * cnt[i]);
            });
          }
        } else {
          float *s = &x[0][0];                 // (VEC == 1)
          int id[MB];
#pragma unroll
          for (int i = 0; i < MB; ++i) id[i] = i;
          bitonic_sort<MB, GRAD>(s, id);       // the indices travel only when the gradient needs them
          if constexpr (GRAD) {
            // mid-rank count difference of every sorted position: a tie run [a, b] has a + b - (M - 1) (a finite
            // member never ties the +inf pads, so no run crosses position M); the pads' own slots are scratch
            int a[MB];
            a[0] = 0;
#pragma unroll
            for (int k = 1; k < MB; ++k) a[k] = s[k] == s[k - 1] ? a[k - 1] : k;
            int b = MB - 1;
#pragma unroll
            for (int k = MB - 1; k >= 0; --k) {
              b = (k + 1 < MB && s[k] == s[k + 1]) ? b : k;
              const float c = (float)(a[k] + b - (M - 1));
              a[k] = __builtin_bit_cast(int, c);
              lds[id[k] * kThreads + tid] = scale * (sgnf(s[k] - yv) * invM - 2.0f * pair_coef * c);
            }
            members<0, MB>(M, [&](auto K_) {
              constexpr int k = decltype(K_)::value;
              pair += __builtin_bit_cast(float, a[k]) * (s[k] - r);
            });
          } else {
            members<0, MB>(M, [&](auto K_) {
              constexpr int k = decltype(K_)::value;
              pair += (float)(2 * k - M + 1) * (s[k] - r);
            });
          }
        }
        pair *= 2.0f;
        const float crps = skill * invM - pair_coef * pair;
        const float err = (r - yv) + dbar;
        acc[0][v] += wn * crps;
        acc[1][v] += wn * (err * err);
        acc[2][v] += wn * (var / varDiv);
        if (grad_target) {
          if constexpr (VEC == 4) y[v] = -scale * invM * sgn_sum;
          else grad_target[off] = -scale * invM * sgn_sum;
        }
      }
      if constexpr (GRAD) {
        float *gp = grad_pred + off;
        members<0, MB>(M, [&](auto I_) {
          constexpr int i = decltype(I_)::value;
          if constexpr (VEC == 4) {
            float4_t g;
#pragma unroll
            for (int v = 0; v < 4; ++v) g[v] = x[i][v];
            *reinterpret_cast<float4_t *>(gp) = g;
          } else if constexpr (SORT) {          // each thread reads back its own column: no barrier
            *gp = lds[i * kThreads + tid];
          } else {
            *gp = x[i][0];
          }
          gp += plane;
          asm volatile("" : "+v"(gp));
        });
      }
      if constexpr (VEC == 4) {
        if (grad_target) {
          float4_t g;
#pragma unroll
          for (int v = 0; v < 4; ++v) g[v] = y[v];
          *reinterpret_cast<float4_t *>(grad_target + off) = g;
        }
      }
    }
  }
  __syncthreads();                              // (the scatter columns are reused below)
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int v = 0; v < VEC; ++v) lds[(q * VEC + v) * kThreads + tid] = acc[q][v];
  __syncthreads();
  if (row == 0 && col < Cv) {
    float *part = ws + 2 + C + (int64_t)blockIdx.y * 3 * C;
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        float s = 0.0f;
        for (int rr = 0; rr < R; ++rr) s += lds[(q * VEC + v) * kThreads + rr * CT + lc];
        part[(int64_t)q * C + col * VEC + v] = s;
      }
  }
}

// scores[q][c] = sum over the node chunks of the partials / sum w; block (c, q), fixed order.  crps_c is also kept in
// ws[2 + c] for the loss.
__global__ __launch_bounds__(kThreads) void k_ens_finish(float *__restrict__ ws, int32_t C, int32_t G,
                                                         float *__restrict__ scores) {
  __shared__ float part[kThreads];
  const int c = blockIdx.x, q = blockIdx.y;
  const float *p = ws + 2 + C + (int64_t)q * C + c;
  float acc = 0.0f;
  for (int g = threadIdx.x; g < G; g += kThreads) acc += p[(int64_t)g * 3 * C];
  block_sum<kThreads>(&part, {acc});
  if (threadIdx.x == 0) {
    const float val = part[0] / ws[0];
    if (q == 0) ws[2 + c] = val;
    if (scores) scores[(int64_t)q * C + c] = val;
  }
}

// loss = sum_c v_c crps_c / sum v; one block, fixed order
__global__ __launch_bounds__(kThreads) void k_ens_loss(const float *__restrict__ ws, const float *__restrict__ chan_w,
                                                       int32_t C, float *__restrict__ loss) {
  __shared__ float part[kThreads];
  float acc = 0.0f;
  for (int c = threadIdx.x; c < C; c += kThreads) acc += (chan_w ? chan_w[c] : 1.0f) * ws[2 + c];
  block_sum<kThreads>(&part, {acc});
  if (threadIdx.x == 0) loss[0] = part[0] / ws[1];
}

// *chunks = the node chunks of the launch, the partials' row count
template <int MB, int VEC, bool SORT, bool GRAD>
int launch_pass(const CrpsArgs &a, int32_t *chunks, hipStream_t st) {
  PassGeometry g;
  const int rc = pass_geometry<&k_ens_crps<MB, VEC, SORT, GRAD>, kThreads>(VEC, a.C, a.N, kMaxChunks, g);
  if (rc != GWEN_OK) return rc;
  *chunks = (int32_t)g.G;
  k_ens_crps<MB, VEC, SORT, GRAD><<<dim3((unsigned)g.gx, (unsigned)g.G), kThreads, 0, st>>>(
      a.pred, a.target, a.node_w, a.chan_w, (int32_t)a.M, a.N, (int32_t)a.C, (int32_t)g.CT, (int32_t)g.R, a.pair_coef,
      a.grad_pred, a.grad_target, a.ws);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

}  // namespace

extern "C" int64_t gwen_ens_crps_workspace_floats(int64_t M, int64_t N, int64_t C) {
  if (M < 1 || M > 64 || N < 1 || C < 1) return 0;
  return 2 + C + 3 * C * (N < kMaxChunks ? N : kMaxChunks);
}

extern "C" int gwen_ens_crps_f32(const float *pred, const float *target, const float *node_w, const float *chan_w,
                                 int64_t M, int64_t N, int64_t C, float pair_coef, float *grad_pred,
                                 float *grad_target, float *loss, float *scores, float *workspace,
                                 int64_t workspace_floats, gwen_stream_t stream_) {
  if (!shape_ok(M, N, C)) return GWEN_EINVAL;
  if (!pred || !target || !loss || !workspace || workspace_floats < gwen_ens_crps_workspace_floats(M, N, C))
    return GWEN_EINVAL;
  if (!aligned_all({pred, target, node_w, chan_w, grad_pred, grad_target, loss, scores, workspace}, 4))
    return GWEN_EINVAL;
  // the 16-byte path: 4 channels per thread (member planes N*C floats apart stay aligned when C % 4 == 0), up to 16
  // members; above, the network holds one point per thread
  const bool vec4 = C % 4 == 0 && aligned_all({pred, target, grad_pred, grad_target}, 16);
  hipStream_t st = gwen_stream(stream_);
  k_ens_weight_sums<<<1, 1024, 0, st>>>(node_w, N, chan_w, C, workspace);
  GWEN_LAUNCH_CHECK();
  const CrpsArgs a{pred, target, node_w, chan_w, M, N, C, pair_coef, grad_pred, grad_target, workspace};
  int32_t G = 0;
  auto pass = [&](auto vec, auto grad) {
    return dispatch_bucket(gwen::ints<4, 8, 16, 32, 64>{}, M, [&](auto mb) {
      constexpr int MB = decltype(mb)::value;
      constexpr bool SORT = MB > 16;
      return launch_pass<MB, SORT ? 1 : decltype(vec)::value, SORT, decltype(grad)::value>(a, &G, st);
    });
  };
  using V4 = std::integral_constant<int, 4>;
  using V1 = std::integral_constant<int, 1>;
  const int rc = vec4 ? (grad_pred ? pass(V4(), std::true_type()) : pass(V4(), std::false_type()))
                      : (grad_pred ? pass(V1(), std::true_type()) : pass(V1(), std::false_type()));
  if (rc != GWEN_OK) return rc;
  k_ens_finish<<<dim3((unsigned)C, 3), kThreads, 0, st>>>(workspace, (int32_t)C, G, scores);
  GWEN_LAUNCH_CHECK();
  k_ens_loss<<<1, kThreads, 0, st>>>(workspace, chan_w, (int32_t)C, loss);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}
