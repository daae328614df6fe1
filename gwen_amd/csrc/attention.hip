// Edge attention: multi-head softmax attention of every target node over its in-edges, with an edge term -- the
// kernel of the graph-transformer block (gwen_amd/attention.py), forward and backward.
//
// BUILD-DEFINED, PARITY UNPINNED (the reference has no attention: its only graph layer is GCNConv); semantics are PyG
// TransformerConv's with edge_dim, restated in fp64 by the tests.  H heads, D = F / H, s(e) / d(e) = source / target of
// stored edge e (edges are stored by target):
//     sc[e,h]  = (1 / sqrt(D)) sum_{c in head h} q[d(e),c] (k[s(e),c] + ee[e,c])
//     p[e,h]   = exp(sc[e,h] - lse[d(e),h]),    lse[d,h] = log sum_{e into d} exp(sc[e,h])
//     out[d,c] = sum_{e into d} p[e,h(c)] (v[s(e),c] + ee[e,c])            (no in-edges: out = 0, lse = -inf)
// The softmax is the running-maximum form: (m, l, acc) are rescaled by exp(m - m') whenever an edge raises the maximum,
// so no logit magnitude overflows; sums run in stored edge order.
//
// One group of G = F / 4 adjacent lanes per TARGET (one 16-byte piece per lane), 256 / G targets a block, as K2 and
// k_layer_norm<.., SEG>; a head is DL = D / 4 adjacent lanes of the group and its dot product a DL-lane butterfly.
// The k / v rows of src[e] are gathers, the ee row of edge e streams.  The loop takes two edges a pass and both edges'
// loads are issued before either is used.  For that the second update must not sit under an `if`: hipcc sinks the
// second edge's loads into the branch, behind the first edge's arithmetic.  So the second update always runs and is
// switched off through its VALUES past the row's end -- a logit of -inf in the forward (a = 1, p = 0: m, l and acc stay as
// they are), a zero weight in the backward -- and its index then falls back to the row's FIRST edge (clamped to the edge
// before it, hipcc proves the two loads equal and makes the second conditional again).
//
// Backward, atomic-free, g = dL/dout, delta[d,h] = sum_{c in h} g[d,c] out[d,c]:
//     dp[e,h] = sum_{c in h} g[d(e),c] (v[s(e),c] + ee[e,c]),     ds[e,h] = p[e,h] (dp[e,h] - delta[d(e),h])
//   pass T (one group per TARGET, the forward's walk; sc and p recomputed from lse):
//     gq[d]  = (1 / sqrt(D)) sum_{e into d} ds[e,h] (k[s(e)] + ee[e]),   gee[e] = (1 / sqrt(D)) ds[e,h] q[d(e)] + p[e,h] g[d(e)],
//     and the two small per-edge arrays P, DS [E, H]
//   pass S (one group per SOURCE over the edge-position CSR of its out-edges, stored order inside a source):
//     gk[s] = (1 / sqrt(D)) sum_{e out of s} ds[e,h] q[d(e)],            gv[s] = sum_{e out of s} p[e,h] g[d(e)]
// q, k, v, gk, gv take a row stride (column blocks of a stacked projection); every row offset is 64-bit.
#include <math.h>
#include <initializer_list>
#include "common.h"

namespace {

constexpr int kThreads = 256;

template <int DL>
__device__ inline float head_sum(float s) {
#pragma unroll
  for (int o = DL / 2; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  return s;
}

__device__ inline float dot4(const float4_t a, const float4_t b) {
  return (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]);
}

__device__ inline float4_t ld4(const float *p) { return *reinterpret_cast<const float4_t *>(p); }
__device__ inline void st4(float *p, const float4_t v) { *reinterpret_cast<float4_t *>(p) = v; }
__device__ inline float4_t splat(float s) { return float4_t{s, s, s, s}; }

template <int G, int DL, bool EE>
__global__ __launch_bounds__(kThreads) void k_attn_fwd(const float *__restrict__ q, int64_t ldq,
                                                       const float *__restrict__ k, int64_t ldk,
                                                       const float *__restrict__ v, int64_t ldv,
                                                       const float *__restrict__ ee, const int32_t *__restrict__ rowptr,
                                                       const int32_t *__restrict__ src, int64_t Nd, float scale,
                                                       float *__restrict__ out, float *__restrict__ lse) {
  constexpr int F = 4 * G, H = G / DL;
  const int lane = threadIdx.x % G, c = 4 * lane;
  const int64_t d = (blockIdx.x * (int64_t)kThreads + threadIdx.x) / G;
  if (d >= Nd) return;                                            // (whole groups: G divides the wave)
  const float4_t qv = ld4(q + d * ldq + c);
  const int32_t s0 = rowptr[d], s1 = rowptr[d + 1];
  float m = -INFINITY, l = 0.0f;
  float4_t acc = splat(0.0f);
  auto edge = [&](float4_t kk, float4_t vv, bool on) {
    const float sc = head_sum<DL>(dot4(qv, kk)) * scale + (on ? 0.0f : -INFINITY);     // (added, not selected: see above)
    const float mn = fmaxf(m, sc);
    const float a = expf(m - mn), p = expf(sc - mn);              // (first edge: a = exp(-inf) = 0; off: a = 1, p = 0)
    l = l * a + p;
    acc = acc * splat(a) + splat(p) * vv;
    m = mn;
  };
  for (int32_t e = s0; e < s1; e += 2) {
    const int32_t e1 = e + 1 < s1 ? e + 1 : s0;                   // past the row: its first edge again (a valid load)
    const int64_t a0 = src[e], a1 = src[e1];
    float4_t k0 = ld4(k + a0 * ldk + c), v0 = ld4(v + a0 * ldv + c);
    float4_t k1 = ld4(k + a1 * ldk + c), v1 = ld4(v + a1 * ldv + c);
    if constexpr (EE) {
      const float4_t x0 = ld4(ee + (int64_t)e * F + c), x1 = ld4(ee + (int64_t)e1 * F + c);
      k0 += x0; v0 += x0; k1 += x1; v1 += x1;
    }
    edge(k0, v0, true);
    edge(k1, v1, e + 1 < s1);
  }
  if (s1 > s0) {
    const float inv = 1.0f / l;
    acc = acc * splat(inv);
  }
  st4(out + d * F + c, acc);
  if (lane % DL == 0) lse[d * H + lane / DL] = s1 > s0 ? m + logf(l) : -INFINITY;
}

template <int G, int DL, bool EE>
__global__ __launch_bounds__(kThreads) void k_attn_bwd_t(const float *__restrict__ q, int64_t ldq,
                                                         const float *__restrict__ k, int64_t ldk,
                                                         const float *__restrict__ v, int64_t ldv,
                                                         const float *__restrict__ ee, const int32_t *__restrict__ rowptr,
                                                         const int32_t *__restrict__ src, const float *__restrict__ g,
                                                         const float *__restrict__ out, const float *__restrict__ lse,
                                                         int64_t Nd, float scale, float *__restrict__ gq,
                                                         float *__restrict__ gee, float *__restrict__ P,
                                                         float *__restrict__ DS) {
  constexpr int F = 4 * G, H = G / DL;
  const int lane = threadIdx.x % G, c = 4 * lane, h = lane / DL;
  const int64_t d = (blockIdx.x * (int64_t)kThreads + threadIdx.x) / G;
  if (d >= Nd) return;
  const float4_t qv = ld4(q + d * ldq + c), gv = ld4(g + d * F + c);
  const float delta = head_sum<DL>(dot4(gv, ld4(out + d * F + c)));
  const float ls = lse[d * H + h];
  const int32_t s0 = rowptr[d], s1 = rowptr[d + 1];
  float4_t acc = splat(0.0f);
  auto edge = [&](int32_t e, float4_t kk, float4_t vv, bool on) {
    const float sc = head_sum<DL>(dot4(qv, kk)) * scale;
    const float p = expf(sc - ls);
    const float ds = p * (head_sum<DL>(dot4(gv, vv)) - delta);
    acc += splat(on ? ds : 0.0f) * kk;
    if (!on) return;                                              // (the stores only: every load is above)
    if constexpr (EE) st4(gee + (int64_t)e * F + c, splat(scale * ds) * qv + splat(p) * gv);
    if (lane % DL == 0) {
      P[(int64_t)e * H + h] = p;
      DS[(int64_t)e * H + h] = ds;
    }
  };
  for (int32_t e = s0; e < s1; e += 2) {
    const int32_t e1 = e + 1 < s1 ? e + 1 : s0;
    const int64_t a0 = src[e], a1 = src[e1];
    float4_t k0 = ld4(k + a0 * ldk + c), v0 = ld4(v + a0 * ldv + c);
    float4_t k1 = ld4(k + a1 * ldk + c), v1 = ld4(v + a1 * ldv + c);
    if constexpr (EE) {
      const float4_t x0 = ld4(ee + (int64_t)e * F + c), x1 = ld4(ee + (int64_t)e1 * F + c);
      k0 += x0; v0 += x0; k1 += x1; v1 += x1;
    }
    edge(e, k0, v0, true);
    edge(e1, k1, v1, e + 1 < s1);
  }
  st4(gq + d * F + c, acc * splat(scale));
}

// one group per SOURCE: rows of (rowptr, col) are the stored positions of its out-edges
template <int G, int DL>
__global__ __launch_bounds__(kThreads) void k_attn_bwd_s(const int32_t *__restrict__ rowptr,
                                                         const int32_t *__restrict__ col,
                                                         const int32_t *__restrict__ dst, const float *__restrict__ q,
                                                         int64_t ldq, const float *__restrict__ g,
                                                         const float *__restrict__ P, const float *__restrict__ DS,
                                                         int64_t Ns, float scale, float *__restrict__ gk, int64_t ldgk,
                                                         float *__restrict__ gv, int64_t ldgv) {
  constexpr int F = 4 * G, H = G / DL;
  const int lane = threadIdx.x % G, c = 4 * lane, h = lane / DL;
  const int64_t s = (blockIdx.x * (int64_t)kThreads + threadIdx.x) / G;
  if (s >= Ns) return;
  const int32_t s0 = rowptr[s], s1 = rowptr[s + 1];
  float4_t ak = splat(0.0f), av = splat(0.0f);
  for (int32_t i = s0; i < s1; i += 2) {
    const int32_t i1 = i + 1 < s1 ? i + 1 : s0;
    const int64_t e0 = col[i], e1 = col[i1];
    const int64_t d0 = dst[e0], d1 = dst[e1];
    const float4_t q0 = ld4(q + d0 * ldq + c), g0 = ld4(g + d0 * F + c);
    const float4_t q1 = ld4(q + d1 * ldq + c), g1 = ld4(g + d1 * F + c);
    const float p0 = P[e0 * H + h], t0 = DS[e0 * H + h];
    const float on = i + 1 < s1 ? 1.0f : 0.0f;                    // (multiplied, not selected: the loads stay unconditional)
    const float p1 = P[e1 * H + h] * on, t1 = DS[e1 * H + h] * on;
    ak += splat(t0) * q0;
    av += splat(p0) * g0;
    ak += splat(t1) * q1;
    av += splat(p1) * g1;
  }
  st4(gk + s * ldgk + c, ak * splat(scale));
  st4(gv + s * ldgv + c, av);
}

inline bool pow2(int64_t x) { return x > 0 && (x & (x - 1)) == 0; }
inline bool fits(int64_t n) { return n < (int64_t(1) << 31); }
inline bool ld_ok(int64_t ld, int64_t F) { return ld >= F && ld % 4 == 0; }
inline bool all_aligned(std::initializer_list<const void *> ps) {
  for (const void *p : ps)
    if (p && !gwen_aligned(p, 16)) return false;
  return true;
}

}  // namespace

// every (G, DL) of gwen_edge_attention_supported: G = F / 4 in {8, 16, 32, 64}, DL = D / 4 a power of two up to G
#define GWEN_ATTN_ALL(X)                                                                                             \
  X(8, 1) X(8, 2) X(8, 4) X(8, 8)                                                                                    \
  X(16, 1) X(16, 2) X(16, 4) X(16, 8) X(16, 16)                                                                      \
  X(32, 1) X(32, 2) X(32, 4) X(32, 8) X(32, 16) X(32, 32)                                                            \
  X(64, 1) X(64, 2) X(64, 4) X(64, 8) X(64, 16) X(64, 32) X(64, 64)

extern "C" int gwen_edge_attention_supported(int64_t F, int64_t H) {
  if (F != 32 && F != 64 && F != 128 && F != 256) return 0;
  return pow2(H) && H <= F / 4 ? 1 : 0;
}

extern "C" int gwen_edge_attention_f32(const float *q, int64_t ldq, const float *k, int64_t ldk, const float *v,
                                       int64_t ldv, const float *ee, const int32_t *rowptr, const int32_t *src,
                                       int64_t Nd, int64_t Ns, int64_t E, int64_t F, int64_t H, float *out, float *lse,
                                       gwen_stream_t stream) {
  if (Nd < 0 || Ns < 0 || E < 0 || !gwen_edge_attention_supported(F, H)) return GWEN_EINVAL;
  if (Nd == 0) return GWEN_OK;
  if (!fits(Nd) || !fits(Ns) || !fits(E)) return GWEN_ERANGE;
  if (!q || !rowptr || !out || !lse || (E > 0 && (!k || !v || !src || Ns == 0))) return GWEN_EINVAL;
  if (!ld_ok(ldq, F) || (E > 0 && (!ld_ok(ldk, F) || !ld_ok(ldv, F)))) return GWEN_EINVAL;
  if (!all_aligned({q, k, v, ee, out}) || !gwen_aligned(lse, 4) || !gwen_aligned(rowptr, 4) || !gwen_aligned(src, 4))
    return GWEN_EINVAL;
  if (out == q || out == k || out == v || out == ee) return GWEN_EINVAL;
  const int G = (int)(F / 4), DL = (int)(F / H / 4);
  const int64_t blocks = (Nd * G + kThreads - 1) / kThreads;
  if (!fits(blocks)) return GWEN_ERANGE;
  const float scale = 1.0f / sqrtf((float)(F / H));
  hipStream_t st = gwen_stream(stream);
#define GWEN_ATTN(GG, DD)                                                                                              \
  if (G == GG && DL == DD) {                                                                                           \
    if (ee) k_attn_fwd<GG, DD, true><<<(unsigned)blocks, kThreads, 0, st>>>(q, ldq, k, ldk, v, ldv, ee, rowptr, src, Nd, scale, out, lse); \
    else k_attn_fwd<GG, DD, false><<<(unsigned)blocks, kThreads, 0, st>>>(q, ldq, k, ldk, v, ldv, nullptr, rowptr, src, Nd, scale, out, lse); \
  }
  GWEN_ATTN_ALL(GWEN_ATTN)
#undef GWEN_ATTN
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

extern "C" int gwen_edge_attention_bwd_target_f32(const float *q, int64_t ldq, const float *k, int64_t ldk,
                                                  const float *v, int64_t ldv, const float *ee, const int32_t *rowptr,
                                                  const int32_t *src, const float *g, const float *out,
                                                  const float *lse, int64_t Nd, int64_t Ns, int64_t E, int64_t F,
                                                  int64_t H, float *gq, float *gee, float *P, float *DS,
                                                  gwen_stream_t stream) {
  if (Nd < 0 || Ns < 0 || E < 0 || !gwen_edge_attention_supported(F, H)) return GWEN_EINVAL;
  if (Nd == 0) return GWEN_OK;
  if (!fits(Nd) || !fits(Ns) || !fits(E)) return GWEN_ERANGE;
  if (!q || !rowptr || !g || !out || !lse || !gq) return GWEN_EINVAL;
  if (E > 0 && (!k || !v || !src || !P || !DS || Ns == 0 || (ee && !gee))) return GWEN_EINVAL;
  if (!ld_ok(ldq, F) || (E > 0 && (!ld_ok(ldk, F) || !ld_ok(ldv, F)))) return GWEN_EINVAL;
  if (!all_aligned({q, k, v, ee, g, out, gq, gee}) || !gwen_aligned(lse, 4) || !gwen_aligned(P, 4) ||
      !gwen_aligned(DS, 4) || !gwen_aligned(rowptr, 4) || !gwen_aligned(src, 4))
    return GWEN_EINVAL;
  if (gq == q || gq == g || gq == out || (gee && (gee == ee || gee == k || gee == v)) || (P && P == DS)) return GWEN_EINVAL;
  const int G = (int)(F / 4), DL = (int)(F / H / 4);
  const int64_t blocks = (Nd * G + kThreads - 1) / kThreads;
  if (!fits(blocks)) return GWEN_ERANGE;
  const float scale = 1.0f / sqrtf((float)(F / H));
  hipStream_t st = gwen_stream(stream);
#define GWEN_ATTN(GG, DD)                                                                                              \
  if (G == GG && DL == DD) {                                                                                           \
    if (ee) k_attn_bwd_t<GG, DD, true><<<(unsigned)blocks, kThreads, 0, st>>>(q, ldq, k, ldk, v, ldv, ee, rowptr, src, g, out, lse, Nd, scale, gq, gee, P, DS); \
    else k_attn_bwd_t<GG, DD, false><<<(unsigned)blocks, kThreads, 0, st>>>(q, ldq, k, ldk, v, ldv, nullptr, rowptr, src, g, out, lse, Nd, scale, gq, nullptr, P, DS); \
  }
  GWEN_ATTN_ALL(GWEN_ATTN)
#undef GWEN_ATTN
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

extern "C" int gwen_edge_attention_bwd_source_f32(const int32_t *src_rowptr, const int32_t *src_col, const int32_t *dst,
                                                  const float *q, int64_t ldq, const float *g, const float *P,
                                                  const float *DS, int64_t Ns, int64_t Nd, int64_t E, int64_t F,
                                                  int64_t H, float *gk, int64_t ldgk, float *gv, int64_t ldgv,
                                                  gwen_stream_t stream) {
  if (Nd < 0 || Ns < 0 || E < 0 || !gwen_edge_attention_supported(F, H)) return GWEN_EINVAL;
  if (Ns == 0) return GWEN_OK;
  if (!fits(Nd) || !fits(Ns) || !fits(E)) return GWEN_ERANGE;
  if (!src_rowptr || !gk || !gv || gk == gv) return GWEN_EINVAL;
  if (E > 0 && (!src_col || !dst || !q || !g || !P || !DS || Nd == 0 || !ld_ok(ldq, F))) return GWEN_EINVAL;
  if (!ld_ok(ldgk, F) || !ld_ok(ldgv, F)) return GWEN_EINVAL;
  if (!all_aligned({q, g, gk, gv}) || !gwen_aligned(P, 4) || !gwen_aligned(DS, 4) || !gwen_aligned(src_rowptr, 4) ||
      !gwen_aligned(src_col, 4) || !gwen_aligned(dst, 4))
    return GWEN_EINVAL;
  const int G = (int)(F / 4), DL = (int)(F / H / 4);
  const int64_t blocks = (Ns * G + kThreads - 1) / kThreads;
  if (!fits(blocks)) return GWEN_ERANGE;
  const float scale = 1.0f / sqrtf((float)(F / H));
  hipStream_t st = gwen_stream(stream);
#define GWEN_ATTN(GG, DD)                                                                                              \
  if (G == GG && DL == DD)                                                                                             \
    k_attn_bwd_s<GG, DD><<<(unsigned)blocks, kThreads, 0, st>>>(src_rowptr, src_col, dst, q, ldq, g, P, DS, Ns, scale, gk, ldgk, gv, ldgv);
  GWEN_ATTN_ALL(GWEN_ATTN)
#undef GWEN_ATTN
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}
