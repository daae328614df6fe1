// Ensemble products and calibration over the members axis of pred [M, N, C] (gwen_amd.products), in the shape of the
// CRPS pass (ensemble.hip): one thread per point, a wave reads 64 consecutive columns of every member plane, no atomics.
//
//   gwen_ens_products_f32: one launch, every point read once, any subset of
//     mean      r + (1/M) sum_i (x_i - r), r = x_0        std   sqrt(sum_i ((x_i - r) - dbar)^2 / (M - 1))
//     prob[t]   #{i : x_i > thr_t} / M                    quantiles[q]   "linear": s[lo] + frac (s[lo + 1] - s[lo])
//   The statistics and the counts come from the members as loaded; the quantiles from a register bitonic network on
//   values alone (min / max, pads of +inf behind the members) that runs after them.  pos, lo and frac of every q are
//   formed once per block and kept in LDS: they are the same in every lane, so the two order statistics are picked by a
//   tree of uniform branches, never by indexing the member registers.
//   gwen_ens_rank_hist_f32: b = #{x_i < y}, t = #{x_i == y} from one sweep over the members (no member registers, no
//   sort); every thread owns M + 1 LDS bins, adds w_n / (t + 1) to bins b..b+t in node order, the block sums its rows in
//   a fixed order into a partial histogram per node chunk, and a finish kernel sums the chunks in a fixed order.
// The member chains, the network, the pass geometry and the bucket dispatch are csrc/members.h's.
#include "members.h"

namespace {

using namespace gwen::ens;

constexpr int kThreads = 256;
constexpr int kMaxTable = 32;                   // quantiles, thresholds of one call
constexpr int kHistMaxChunks = 1024;            // node chunks of the rank histogram, and
constexpr int64_t kHistMaxFloats = 1 << 22;     // ... of its partials: chunks * C * (M + 1) floats, 16 MiB

// a = s[lo], b = s[lo + 1] for a wave-uniform lo in [L, H): a binary tree of uniform branches over register indices
template <int L, int H, int MB>
__device__ __forceinline__ void pick(const float (&s)[MB], int lo, float &a, float &b) {
  if constexpr (H - L == 1) {
    a = s[L];
    b = s[L + 1 < MB ? L + 1 : L];
    // (an empty asm per leaf: without it the compiler sinks the leaves' loads into one load at a variable index, and the
    // member registers become an LDS or scratch array)
    asm volatile("" : "+v"(a), "+v"(b));
  } else {
    constexpr int mid = (L + H) / 2;
    if (lo < mid) pick<L, mid, MB>(s, lo, a, b);
    else pick<mid, H, MB>(s, lo, a, b);
  }
}

// The products pass.  Thread (row, lc) of block (bx, by) owns VEC consecutive channels (vector column bx * CT + lc) and
// walks the nodes n = by * R + row, += gridDim.y * R, as k_ens_crps.  MB: the member bucket (M <= MB); SORT: quantiles
// wanted (VEC == 1).  Every output element is a function of its own point only, by the same operations in the same
// order whatever VEC is: the two paths give the same bits.
template <int MB, int VEC, bool SORT>
__global__ __launch_bounds__(kThreads) void k_ens_products(const float *__restrict__ pred, int32_t M_, int64_t N,
                                                           int32_t C, int32_t CT, int32_t R,
                                                           const float *__restrict__ q, int32_t Q,
                                                           const float *__restrict__ thr, int32_t T,
                                                           int32_t thr_per_channel, float *__restrict__ mean,
                                                           float *__restrict__ stdv, float *__restrict__ quant,
                                                           float *__restrict__ prob) {
  static_assert(!SORT || VEC == 1, "the sorting network holds one point per thread");
  __shared__ int s_lo[kMaxTable];
  __shared__ float s_frac[kMaxTable];
  const int tid = threadIdx.x;
  if (SORT && tid < Q) {
    // pos is rounded once, in fp32; a q outside [0, 1] (or NaN) gives NaN through frac
    const float qv = q[tid];
    const float pos = qv * (float)(M_ - 1);
    const float fl = __builtin_floorf(pos);
    const bool ok = qv >= 0.0f && qv <= 1.0f;
    s_lo[tid] = ok ? (int)fl : 0;
    s_frac[tid] = ok ? pos - fl : __builtin_nanf("");
  }
  __syncthreads();
  const int row = tid / CT, lc = tid - row * CT;
  const int Cv = VEC == 4 ? C / 4 : C;
  const int64_t col = (int64_t)blockIdx.x * CT + lc;
  if (!(row < R && col < Cv)) return;
  const int64_t plane_ = N * (int64_t)C;
  const float fM = (float)M_;
  const float invM = 1.0f / fM;
  const float varDiv = (float)(M_ - 1);               // M = 1: 0 / 0 = NaN, torch's unbiased std of one value
  for (int64_t n = (int64_t)blockIdx.y * R + row; n < N; n += (int64_t)gridDim.y * R) {
    int M = M_;
    int64_t plane = plane_;
    fresh(M, plane);
    const int64_t off = n * C + col * VEC;
    float x[VEC][MB];
    {
      // the member loads: the element OFFSET passes the empty asm here (the loads stay global loads, which a laundered
      // pointer's do not), the pointer in k_ens_crps -- two bodies on purpose
      int64_t o = off;
      members<0, MB>(fresh(M), [&](auto I_) {
        constexpr int i = decltype(I_)::value;
        if constexpr (VEC == 4) {
          const float4_t p = *reinterpret_cast<const float4_t *>(pred + o);
#pragma unroll
          for (int v = 0; v < 4; ++v) x[v][i] = p[v];
        } else {
          x[0][i] = pred[o];
        }
        o += plane;
        asm volatile("" : "+v"(o));
      });
      // pads of +inf sort behind every member
      if constexpr (SORT) pads<MB - 1>(fresh(M), [&](auto I_) { x[0][decltype(I_)::value] = __builtin_inff(); });
    }
    if (mean || stdv) {
      float mu[VEC], sd[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const float r = x[v][0];
        float dsum = 0.0f, var = 0.0f;          // (as in k_ens_crps, where dsum shares a chain with the skill: two bodies)
        members<0, MB>(fresh(M), [&](auto I_) {
          constexpr int i = decltype(I_)::value;
          dsum += x[v][i] - r;
        });
        const float dbar = dsum * invM;
        members<0, MB>(fresh(M), [&](auto I_) {
          constexpr int i = decltype(I_)::value;
          const float t = (x[v][i] - r) - dbar;
          var += t * t;
        });
        mu[v] = r + dbar;
        sd[v] = __builtin_sqrtf(var / varDiv);
      }
      if constexpr (VEC == 4) {
        if (mean) *reinterpret_cast<float4_t *>(mean + off) = float4_t{mu[0], mu[1], mu[2], mu[3]};
        if (stdv) *reinterpret_cast<float4_t *>(stdv + off) = float4_t{sd[0], sd[1], sd[2], sd[3]};
      } else {
        if (mean) mean[off] = mu[0];
        if (stdv) stdv[off] = sd[0];
      }
    }
    if (T > 0) {
      int64_t o = off;
      for (int t = 0; t < T; ++t) {
        float pr[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const float tv = thr[thr_per_channel ? (int64_t)t * C + col * VEC + v : (int64_t)t];
          float cnt = 0.0f;                     // NaN > tv is false: a NaN member does not exceed
          members<0, MB>(fresh(M), [&](auto I_) {
            constexpr int i = decltype(I_)::value;
            cnt += x[v][i] > tv ? 1.0f : 0.0f;
            __builtin_amdgcn_sched_barrier(0);  // a compare's lane mask is used at once: MB masks up front spill
          });
          pr[v] = cnt / fM;
        }
        if constexpr (VEC == 4) *reinterpret_cast<float4_t *>(prob + o) = float4_t{pr[0], pr[1], pr[2], pr[3]};
        else prob[o] = pr[0];
        o += plane;
      }
    }
    if constexpr (SORT) {
      float(&s)[MB] = x[0];
      // min / max drop a NaN silently: a flag carries it (the largest |bits| of the point, no lane mask per member)
      uint32_t top = 0;
      members<0, MB>(fresh(M), [&](auto I_) {
        constexpr int i = decltype(I_)::value;
        const uint32_t mag = __builtin_bit_cast(uint32_t, s[i]) & 0x7fffffffu;
        top = mag > top ? mag : top;
      });
      const bool has_nan = top > 0x7f800000u;
      bitonic_sort<MB, false>(s);
      int64_t o = off;
      for (int qi = 0; qi < Q; ++qi) {
        const int lo = __builtin_amdgcn_readfirstlane(s_lo[qi]);
        const float frac = s_frac[qi];
        float a, b;
        pick<0, MB, MB>(s, lo, a, b);
        // frac == 0 copies the order statistic: no arithmetic, an infinite minimum / maximum comes back as it is
        float val = frac == 0.0f ? a : a + frac * (b - a);
        val = has_nan ? __builtin_nanf("") : val;
        quant[o] = val;
        o += plane;
      }
    }
  }
}

// A validated call, as gwen_ens_products_f32 names its arguments: what the dispatch hands to launch_products.  (The kernel
// keeps a parameter list, as k_ens_crps does: csrc/ensemble.hip.)
struct ProductsArgs {
  const float *pred;
  int64_t M, N, C;
  const float *q;
  int64_t Q;
  const float *thr;
  int64_t T;
  int thr_per_channel;
  float *mean, *stdv, *quant, *prob;
};

template <int MB, int VEC, bool SORT>
int launch_products(const ProductsArgs &a, hipStream_t st) {
  PassGeometry g;                               // nothing is summed over the chunks: up to the grid's own limit
  const int rc = pass_geometry<&k_ens_products<MB, VEC, SORT>, kThreads>(VEC, a.C, a.N, 65535, g);
  if (rc != GWEN_OK) return rc;
  k_ens_products<MB, VEC, SORT><<<dim3((unsigned)g.gx, (unsigned)g.G), kThreads, 0, st>>>(
      a.pred, (int32_t)a.M, a.N, (int32_t)a.C, (int32_t)g.CT, (int32_t)g.R, a.q, (int32_t)a.Q, a.thr, (int32_t)a.T,
      a.thr_per_channel, a.mean, a.stdv, a.quant, a.prob);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

// the member bucket; the 16-byte path (VEC == 4) holds up to 16 members
template <int VEC, bool SORT>
int dispatch_products(const ProductsArgs &a, hipStream_t st) {
  return dispatch_bucket(gwen::ints<4, 8, 16, 32, 64>{}, a.M, [&](auto mb) {
    constexpr int MB = decltype(mb)::value;
    return launch_products<MB, (MB > 16 ? 1 : VEC), SORT>(a, st);
  });
}

// Node chunks of the rank histogram: a function of the shapes alone (not of the device or of a pointer's alignment),
// so that the order of every sum is too.
struct HistShape {
  int64_t threads;
  ColumnTiles t;
  int64_t G;
};

HistShape hist_shape(int64_t M, int64_t N, int64_t C) {
  HistShape h;
  h.threads = M <= 32 ? 256 : 128;              // (M + 1) LDS bins a thread: at most 33 KiB a block
  h.t = column_tiles(C, h.threads);
  int64_t G = (N + h.t.R - 1) / h.t.R;
  const int64_t fit = kHistMaxFloats / (C * (M + 1));
  G = G < kHistMaxChunks ? G : kHistMaxChunks;
  G = G < fit ? G : (fit < 1 ? 1 : fit);
  h.G = G;
  return h;
}

// Thread (row, lc) of block (bx, by) owns channel bx * CT + lc and the LDS bins lds[k * blockDim.x + tid], k <= M; it
// walks the nodes n = by * R + row, += gridDim.y * R.  part[by][c][k] = the block's rows summed in row order.
__global__ __launch_bounds__(kThreads) void k_ens_rank_hist(const float *__restrict__ pred,
                                                            const float *__restrict__ target,
                                                            const float *__restrict__ node_w, int32_t M, int64_t N,
                                                            int32_t C, int32_t CT, int32_t R,
                                                            float *__restrict__ part) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int nb = M + 1;
  for (int k = 0; k < nb; ++k) lds[k * nt + tid] = 0.0f;
  const int row = tid / CT, lc = tid - row * CT;
  const int64_t c = (int64_t)blockIdx.x * CT + lc;
  const int64_t plane = N * (int64_t)C;
  if (row < R && c < C) {
    for (int64_t n = (int64_t)blockIdx.y * R + row; n < N; n += (int64_t)gridDim.y * R) {
      const int64_t off = n * C + c;
      const float y = target[off];
      const float *pp = pred + off;
      int b = 0, t = 0;
      bool bad = y != y;
#pragma unroll 8
      for (int i = 0; i < M; ++i) {
        const float xi = *pp;
        pp += plane;
        b += xi < y ? 1 : 0;
        t += xi == y ? 1 : 0;
        bad |= xi != xi;
      }
      if (!bad) {
        const float wn = node_w ? node_w[n] : 1.0f;
        const float share = wn / (float)(t + 1);       // the mid-rank split: the expectation of random tie-breaking
        for (int k = b; k <= b + t; ++k) lds[k * nt + tid] += share;
      }
    }
  }
  __syncthreads();
  if (row == 0 && c < C) {
    float *out = part + ((int64_t)blockIdx.y * C + c) * nb;
    for (int k = 0; k < nb; ++k) {
      float s = 0.0f;
      for (int rr = 0; rr < R; ++rr) s += lds[k * nt + rr * CT + lc];
      out[k] = s;
    }
  }
}

// hist[c][k] = sum over the node chunks of part[g][c][k]; block c.  256 / (M + 1) slots of M + 1 threads take every
// slots-th chunk each (a chunk's bins are contiguous), then bin k sums its slots in order; normalize divides the row by
// its own sum, taken in bin order by every thread alike.
__global__ __launch_bounds__(kThreads) void k_ens_rank_hist_finish(const float *__restrict__ part, int32_t M, int32_t C,
                                                                   int32_t G, int32_t normalize,
                                                                   float *__restrict__ hist) {
  __shared__ float acc[kThreads];
  __shared__ float rowv[kThreads];
  const int nb = M + 1, slots = kThreads / nb;
  const int tid = threadIdx.x, slot = tid / nb, k = tid - slot * nb;
  const int64_t c = blockIdx.x;
  float a = 0.0f;
  if (slot < slots)
    for (int g = slot; g < G; g += slots) a += part[((int64_t)g * C + c) * nb + k];
  acc[tid] = a;
  __syncthreads();
  if (tid < nb) {
    float s = 0.0f;
    for (int j = 0; j < slots; ++j) s += acc[j * nb + tid];
    rowv[tid] = s;
  }
  __syncthreads();
  if (tid < nb) {
    float v = rowv[tid];
    if (normalize) {
      float tot = 0.0f;
      for (int j = 0; j < nb; ++j) tot += rowv[j];
      v = v / tot;                              // a row that counted nothing: 0 / 0 = NaN
    }
    hist[c * nb + tid] = v;
  }
}

}  // namespace

extern "C" int gwen_ens_products_f32(const float *pred, int64_t M, int64_t N, int64_t C, const float *q, int64_t Q,
                                     const float *thr, int64_t T, int thr_per_channel, float *mean, float *stdv,
                                     float *quant, float *prob, gwen_stream_t stream_) {
  if (!shape_ok(M, N, C) || Q < 0 || Q > kMaxTable || T < 0 || T > kMaxTable) return GWEN_EINVAL;
  if (!pred || (Q > 0 && (!q || !quant)) || (T > 0 && (!thr || !prob))) return GWEN_EINVAL;
  if (thr_per_channel != 0 && thr_per_channel != 1) return GWEN_EINVAL;
  if (!mean && !stdv && Q == 0 && T == 0) return GWEN_EINVAL;       // nothing asked for
  if (!aligned_all({pred, q, thr, mean, stdv, quant, prob}, 4)) return GWEN_EINVAL;
  if (Q == 0) quant = nullptr;
  if (T == 0) prob = nullptr;
  // the 16-byte path: 4 channels per thread, for the work that needs no sort, while 4 points of members fit in
  // registers (16 members, as the CRPS)
  const bool vec4 = Q == 0 && M <= 16 && C % 4 == 0 && aligned_all({pred, mean, stdv, prob}, 16);
  const ProductsArgs a{pred, M, N, C, q, Q, thr, T, thr_per_channel, mean, stdv, quant, prob};
  hipStream_t st = gwen_stream(stream_);
  if (Q > 0) return dispatch_products<1, true>(a, st);
  if (vec4) return dispatch_products<4, false>(a, st);
  return dispatch_products<1, false>(a, st);
}

extern "C" int64_t gwen_ens_rank_hist_workspace_floats(int64_t M, int64_t N, int64_t C) {
  if (!shape_ok(M, N, C)) return 0;
  return hist_shape(M, N, C).G * C * (M + 1);
}

extern "C" int gwen_ens_rank_hist_f32(const float *pred, const float *target, const float *node_w, int64_t M,
                                      int64_t N, int64_t C, int normalize, float *hist, float *workspace,
                                      int64_t workspace_floats, gwen_stream_t stream_) {
  if (!shape_ok(M, N, C)) return GWEN_EINVAL;
  if (!pred || !target || !hist || !workspace || workspace_floats < gwen_ens_rank_hist_workspace_floats(M, N, C))
    return GWEN_EINVAL;
  if (!aligned_all({pred, target, node_w, hist, workspace}, 4)) return GWEN_EINVAL;
  const HistShape h = hist_shape(M, N, C);
  hipStream_t st = gwen_stream(stream_);
  const size_t lds_bytes = (size_t)h.threads * (size_t)(M + 1) * sizeof(float);
  k_ens_rank_hist<<<dim3((unsigned)h.t.gx, (unsigned)h.G), (unsigned)h.threads, lds_bytes, st>>>(
      pred, target, node_w, (int32_t)M, N, (int32_t)C, (int32_t)h.t.CT, (int32_t)h.t.R, workspace);
  GWEN_LAUNCH_CHECK();
  k_ens_rank_hist_finish<<<(unsigned)C, kThreads, 0, st>>>(workspace, (int32_t)M, (int32_t)C, (int32_t)h.G,
                                                           normalize, hist);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}
