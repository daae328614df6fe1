// Counter-based Gaussian noise for ensemble members (include/gwen_hip.h, "Latent noise"):
//     z(seed, tag, draw, member, node, k) = Box-Muller of the Philox4x64-10 block with key (seed, tag) and counter
//     (node, member, draw, k / 8), so member m's noise is a pure function of its global index and never of the rank,
//     the batching or a graph capture.  The state {seed, draw} is read from device memory: a captured step picks up
//     the current draw on every replay, and gwen_noise_advance moves it in stream order.
// Three launchers: the noise itself ([members, nodes, K]), the fused injection out = x + z Wz^T (one read and one
// write of the latents; z never reaches memory) and the counter advance.  Fixed-order fp32 arithmetic, no atomics.
#include "common.h"

namespace {

constexpr uint64_t kM0 = 0xD2E7470EE14C6C93ull, kM1 = 0xCA5A826395121157ull;    // Philox4x64 multipliers
constexpr uint64_t kW0 = 0x9E3779B97F4A7C15ull, kW1 = 0xBB67AE8584CAA73Bull;    // ... and key increments

// Philox4x64-10 (Salmon et al., SC'11; numpy.random.Philox): c is the counter on entry and the block on exit
__device__ inline void philox4x64_10(uint64_t c[4], uint64_t k0, uint64_t k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    if (i) {
      k0 += kW0;
      k1 += kW1;
    }
    const uint64_t lo0 = kM0 * c[0], hi0 = __umul64hi(kM0, c[0]);
    const uint64_t lo1 = kM1 * c[2], hi1 = __umul64hi(kM1, c[2]);
    const uint64_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = lo1;
    c[2] = n2;
    c[3] = lo0;
  }
}

// Two normals from one 64-bit word: u = ((h >> 8) + 1/2) 2^-24 of its halves, radius from the low half, angle from the
// high one.  u itself needs 25 bits from u = 1/2 up, so ln u comes from u or from 1 - u (whichever is exact in fp32),
// and the angle 2u from 2u or 2u - 2 (period 2 of sincospi): both stay accurate as u -> 1.
__device__ inline void box_muller(uint64_t w, float &za, float &zb) {
  const uint32_t a = (uint32_t)w >> 8, b = (uint32_t)(w >> 32) >> 8;
  const float ln = a < (1u << 23) ? logf(((float)a + 0.5f) * 0x1p-24f)
                                  : log1pf(-(((float)((1u << 24) - 1u - a) + 0.5f) * 0x1p-24f));
  const float r = sqrtf(-2.0f * ln);
  const float t = b < (1u << 23) ? (float)(2u * b + 1u) * 0x1p-24f : -(float)(2u * ((1u << 24) - 1u - b) + 1u) * 0x1p-24f;
  float s, c;
  sincospif(t, &s, &c);
  za = r * c;
  zb = r * s;
}

// z[8 blk .. 8 blk + 7] of (node, member) at the state's draw
__device__ inline void normal8(uint64_t seed, uint64_t tag, uint64_t draw, uint64_t member, uint64_t node,
                               uint64_t blk, float z[8]) {
  uint64_t c[4] = {node, member, draw, blk};
  philox4x64_10(c, seed, tag);
#pragma unroll
  for (int p = 0; p < 4; ++p) box_muller(c[p], z[2 * p], z[2 * p + 1]);
}

constexpr int kThreads = 256;

// one thread per (member, node, block of 8 channels)
__global__ __launch_bounds__(kThreads) void k_noise_normal(const uint64_t *__restrict__ state, uint64_t tag,
                                                           uint64_t member0, int64_t members, int64_t nodes, int64_t K,
                                                           float *__restrict__ out) {
  const int64_t nb = (K + 7) / 8, total = members * nodes * nb;
  const uint64_t seed = state[0], draw = state[1];
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int64_t b = i % nb, mn = i / nb, n = mn % nodes, m = mn / nodes;
    float z[8];
    normal8(seed, tag, draw, member0 + (uint64_t)m, (uint64_t)n, (uint64_t)b, z);
    float *o = out + mn * K + b * 8;
    const int64_t cnt = K - b * 8 < 8 ? K - b * 8 : 8;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < cnt) o[j] = z[j];
  }
}

// wave-scope LDS hand-over between lanes of one wave (release, wave barrier, acquire)
__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The injection.  Block (bx, by): 4 waves, columns [256 by, 256 by + 256) of every row (one float4 per lane), Wz of
// those columns transposed into LDS (wT[k][lane] = Wz[4 lane .. 4 lane + 3, k]).  A wave takes G = 64 / (K / 8) rows at
// a time: lane l computes Philox block l % (K / 8) of row l / (K / 8) -- all 64 lanes busy -- and leaves its 8 normals
// in the wave's LDS slice; then R rows at a time, every lane loads its float4 of the R rows of x, accumulates
// acc[r] = sum_k z[r][k] Wz[:, k] over k in order while those loads are in flight (fmaf from zero, z a broadcast read)
// and writes x + acc.  R rows share each Wz read.
template <int K>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4))) void k_noise_inject(const uint64_t *__restrict__ state, uint64_t member0,
                                                           int64_t rows, int64_t nodes, const float *x,
                                                           const float *__restrict__ wz, int32_t H, float *out) {
  constexpr int NB = K / 8, G = 64 / NB, R = G < 8 ? G : 8;
  __shared__ float4_t wT[K][64];
  __shared__ __attribute__((aligned(16))) float zs[kThreads / 64][G * K];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t h0 = (int64_t)blockIdx.y * 256;
  {                                                  // Wz rows h0 .. h0 + 255 as float4 along k, all loads in flight
    float *wt = reinterpret_cast<float *>(&wT[0][0]);  // wt[k * 256 + h - h0]
    float4_t v[K / 4];
#pragma unroll
    for (int j = 0; j < K / 4; ++j) {
      const int i = tid + j * kThreads, hl = i / (K / 4), k4 = i % (K / 4);
      const int64_t h = h0 + hl < H ? h0 + hl : H - 1;          // (a clamped row, zeroed below: no branch per load)
      v[j] = *reinterpret_cast<const float4_t *>(wz + h * K + 4 * k4);
      if (h0 + hl >= H) v[j] = float4_t{0.0f, 0.0f, 0.0f, 0.0f};
    }
#pragma unroll
    for (int j = 0; j < K / 4; ++j) {
      const int i = tid + j * kThreads, hl = i / (K / 4), k4 = i % (K / 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) wt[(4 * k4 + e) * 256 + hl] = v[j][e];
    }
  }
  __syncthreads();
  const uint64_t seed = state[0], draw = state[1];
  const int64_t col = h0 + 4 * lane;
  const bool on = col < H;
  float *zw = zs[wave];
  for (int64_t r0 = ((int64_t)blockIdx.x * (kThreads / 64) + wave) * G; r0 < rows;
       r0 += (int64_t)gridDim.x * (kThreads / 64) * G) {
    {
      const int64_t r = r0 + lane / NB;
      if (r < rows) {
        float z[8];
        normal8(seed, 0, draw, member0 + (uint64_t)(r / nodes), (uint64_t)(r % nodes), (uint64_t)(lane % NB), z);
        float4_t *dst = reinterpret_cast<float4_t *>(zw + lane * 8);
        dst[0] = float4_t{z[0], z[1], z[2], z[3]};
        dst[1] = float4_t{z[4], z[5], z[6], z[7]};
      }
    }
    wave_sync();
    for (int rc = 0; rc < G; rc += R) {
      // the chunk's x rows are loaded before the k loop (all R in flight while it runs) and stored after it: each lane
      // reads and writes only its own float4 of each row, so out may be x
      float4_t xv[R], acc[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t row = r0 + rc + r;
        acc[r] = float4_t{0.0f, 0.0f, 0.0f, 0.0f};
        xv[r] = acc[r];
        if (on && row < rows) xv[r] = *reinterpret_cast<const float4_t *>(x + row * H + col);
      }
#pragma unroll 1
      for (int k = 0; k < K; k += 4) {
        const float4_t w0 = wT[k][lane], w1 = wT[k + 1][lane], w2 = wT[k + 2][lane], w3 = wT[k + 3][lane];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float4_t z4 = *reinterpret_cast<const float4_t *>(zw + (rc + r) * K + k);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[r][e] = fmaf(z4[0], w0[e], acc[r][e]);
            acc[r][e] = fmaf(z4[1], w1[e], acc[r][e]);
            acc[r][e] = fmaf(z4[2], w2[e], acc[r][e]);
            acc[r][e] = fmaf(z4[3], w3[e], acc[r][e]);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t row = r0 + rc + r;
        if (on && row < rows) *reinterpret_cast<float4_t *>(out + row * H + col) = xv[r] + acc[r];
      }
    }
    wave_sync();                                     // the next group's normals overwrite this group's
  }
}

__global__ void k_noise_advance(uint64_t *state, int64_t n) { state[1] = state[1] + (uint64_t)n; }

int blocks_for(int64_t work, int64_t per_block) {
  const int64_t b = (work + per_block - 1) / per_block;
  return (int)(b < 8192 ? (b > 0 ? b : 1) : 8192);     // grid-stride beyond: 32 blocks of 256 per CU
}

}  // namespace

extern "C" int gwen_noise_normal_f32(const uint64_t *state, uint64_t tag, int64_t member0, int64_t members,
                                     int64_t nodes, int64_t K, float *out, gwen_stream_t stream) {
  if (!state || !gwen_aligned(state, 8) || member0 < 0 || members < 0 || nodes < 0 || K < 1) return GWEN_EINVAL;
  if (members > 0 && nodes > 0 && (!out || !gwen_aligned(out, 4))) return GWEN_EINVAL;
  if (members > 0 && nodes > 0 && (members > INT64_MAX / nodes / ((K + 7) / 8 * 8))) return GWEN_ERANGE;
  const int64_t work = members * nodes * ((K + 7) / 8);
  if (work == 0) return GWEN_OK;
  k_noise_normal<<<blocks_for(work, kThreads), kThreads, 0, gwen_stream(stream)>>>(state, tag, (uint64_t)member0,
                                                                                   members, nodes, K, out);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

extern "C" int gwen_noise_inject_f32(const uint64_t *state, int64_t member0, int64_t rows, int64_t nodes,
                                     const float *x, const float *wz, int64_t H, int64_t K, float *out,
                                     gwen_stream_t stream) {
  if (!state || !gwen_aligned(state, 8) || member0 < 0 || rows < 0 || nodes < 1) return GWEN_EINVAL;
  if (!(K == 8 || K == 16 || K == 32 || K == 64) || H < 4 || H % 4 != 0) return GWEN_EINVAL;
  if (rows > 0 && (!x || !wz || !out || !gwen_aligned(x, 16) || !gwen_aligned(out, 16) || !gwen_aligned(wz, 16)))
    return GWEN_EINVAL;
  if (H > (1 << 30) || rows > INT64_MAX / H) return GWEN_ERANGE;
  if (rows == 0) return GWEN_OK;
  const int64_t G = 64 / (K / 8);
  const int64_t ty = (H + 255) / 256;
  if (ty > 65535) return GWEN_ERANGE;
  const dim3 grid((unsigned)blocks_for(rows, G * (kThreads / 64)), (unsigned)ty);
  hipStream_t st = gwen_stream(stream);
  const uint64_t m0 = (uint64_t)member0;
  switch (K) {
    case 8: k_noise_inject<8><<<grid, kThreads, 0, st>>>(state, m0, rows, nodes, x, wz, (int32_t)H, out); break;
    case 16: k_noise_inject<16><<<grid, kThreads, 0, st>>>(state, m0, rows, nodes, x, wz, (int32_t)H, out); break;
    case 32: k_noise_inject<32><<<grid, kThreads, 0, st>>>(state, m0, rows, nodes, x, wz, (int32_t)H, out); break;
    default: k_noise_inject<64><<<grid, kThreads, 0, st>>>(state, m0, rows, nodes, x, wz, (int32_t)H, out); break;
  }
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

extern "C" int gwen_noise_advance(uint64_t *state, int64_t n, gwen_stream_t stream) {
  if (!state || !gwen_aligned(state, 8)) return GWEN_EINVAL;
  k_noise_advance<<<1, 1, 0, gwen_stream(stream)>>>(state, n);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}
