// U-Net backward kernels (gwen_amd.models_cnn with grad=True):
//   gwen_conv3x3_grad_weight_f32    gW[co][ci][ky][kx] = sum_{b,y,x} g[b,y,x,co] x[b,y+ky-1,x+kx-1,ci], the 3x3 weight
//                                   gradient, on the split contractions of split.h;
//   gwen_upsample2x_backward_f32    the adjoint of gwen_upsample2x_f32 as a gather, with an optional ReLU mask;
//   gwen_norm_relu_backward_f32     ReLU + BatchNorm backward (train or eval), the two channel sums in fp64;
//   gwen_unpool2x2_f32              the max-pool's gradient scattered back by the forward's argmax.
// The data gradient of the convolution is gwen_conv3x3_f32 itself with the weight packed as the other layer type.
//
// The weight-gradient kernel.  v_mfma_f32_16x16x32_bf16 with K = PIXELS: D rows are 16 output channels (A = g), D
// columns 16 input channels (B = x).  A block walks a chunk of 8 x 16 pixel tiles; per tile it stages the 10 x 18 halo
// patch of x and the 8 x 16 tile of g in LDS in the forward's form -- [pixel][32 channels], pixel pitch 96 B, cut into
// the NS bf16 images on the way in -- and each wave owns ONE (16 co) x (16 ci) tile of the block's (up to 2 x 2) for
// all nine taps: 36 accumulator registers.  A k-step is 32 pixels = two tile rows; a lane's fragment is 8 consecutive
// pixels of a row for one channel, which the channels-last image gives through ds_read_b64_tr_b16 (4 pixels x 16
// channels per 16-lane group, lane i gets channel i): two reads per fragment, a tap's (ky, kx) a row-address offset.
// Every lane supplies an in-bounds, 8-byte aligned address and the block is whole waves: EXEC is all ones.
// Pixels outside the image and channels beyond Cin / Cout enter LDS as zeros by a select; memory there is never read.
// Every chunk writes its raw sums exactly once, in the layer's weight layout, to its slab (or, with one chunk, to gW);
// gwen_reduce_chunks_batched adds the slabs in chunk order.  No atomics; element offsets are 64-bit.
#include "conv_common.h"

namespace {

constexpr int kGTile = TH * TW;

struct WgradArgs {
  const float *g, *x;
  float *dst;                      // slab 0 (chunks > 1) or gW
  int32_t H, W, Cin, Cout, tiles_x, tiles_y, gci, nci, transposed, vecg, vecx;
  int64_t ldg, ldx, tiles, tpc, count;
};

// A lane's 8 k-values (consecutive pixels p0 .. p0 + 7 of one image row) of channel c0 + (lane & 15)
__device__ inline bf16x8 frag_pixels(const __bf16 *img, int p0, int c0, int lane) {
#ifdef GWEN_WGRAD_PLAIN_READS
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = img[(p0 + j) * PITCH + c0 + (lane & 15)];
  return v;
#else
  // lane 4 q + p of a 16-lane group: the address of pixel (row) q, channels 4 p .. 4 p + 3; it receives channel
  // (lane & 15) of the four pixels
  const int q = (lane >> 2) & 3, p = lane & 3;
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  const __bf16 *a0 = img + (p0 + q) * PITCH + c0 + 4 * p;
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4 *)(a0));
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4 *)(a0 + 4 * PITCH));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#endif
}

// (pixel, channel quad) items of one staged image: fp32 from memory (zeros outside), split, parked as bf16x4
template <int NS>
__device__ inline void stage_quad(const float *src, bool inside, int c, int C, bool vec, __bf16 *img, int stride, int off) {
  float f4[4] = {0.f, 0.f, 0.f, 0.f};
  if (inside && c < C) {
    if (vec) {                                               // C % 4 == 0: a quad is inside or outside as a whole
      const float4_t v = *reinterpret_cast<const float4_t *>(src);
      f4[0] = v[0]; f4[1] = v[1]; f4[2] = v[2]; f4[3] = v[3];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c + e < C) f4[e] = src[e];
    }
  }
  bf16x4 im[NS];
  gwen::split_images<4, NS>(f4, im);
#pragma unroll
  for (int s = 0; s < NS; ++s) *reinterpret_cast<bf16x4 *>(img + s * stride + off) = im[s];
}

template <int NS>
__global__ __launch_bounds__(kThreads) void k_conv3x3_wgrad(const WgradArgs a) {
  __shared__ __attribute__((aligned(16))) __bf16 ximg[NS * kPatch * PITCH];
  __shared__ __attribute__((aligned(16))) __bf16 gimg[NS * kGTile * PITCH];
  constexpr int kXImg = kPatch * PITCH, kGImg = kGTile * PITCH;
  const int nthreads = blockDim.x;                           // 64 x (channel tiles of this block): whole waves
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, mi = lane & 15, mh = lane >> 4;
  const int tco = wave / a.nci, tci = wave - tco * a.nci;    // this wave's tile of the block's nco x nci
  const int nco = nthreads / (64 * a.nci);
  const int gco = blockIdx.y / a.gci, gcix = blockIdx.y - gco * a.gci;
  const int co0 = gco * nco * 16, ci0 = gcix * a.nci * 16;   // the block's first channels
  const int qx = 4 * a.nci, qg = 4 * nco;                    // channel quads staged per pixel

  f32x4 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int64_t t_lo = blockIdx.x * a.tpc, t_hi = t_lo + a.tpc < a.tiles ? t_lo + a.tpc : a.tiles;
  for (int64_t tile = t_lo; tile < t_hi; ++tile) {
    const int tx = (int)(tile % a.tiles_x), ty = (int)((tile / a.tiles_x) % a.tiles_y);
    const int64_t b = tile / ((int64_t)a.tiles_x * a.tiles_y);
    const int y0 = ty * TH, x0 = tx * TW;
    const float *xb = a.x + b * a.H * a.W * a.ldx, *gb = a.g + b * a.H * a.W * a.ldg;
    for (int idx = threadIdx.x; idx < kPatch * qx; idx += nthreads) {
      const int p = idx / qx, kq = (idx - p * qx) * 4;
      const int py = p / PW, px = p - py * PW;
      const int gy = y0 - 1 + py, gx = x0 - 1 + px, c = ci0 + kq;
      const bool inside = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
      stage_quad<NS>(xb + ((int64_t)gy * a.W + gx) * a.ldx + c, inside, c, a.Cin, a.vecx, ximg, kXImg, p * PITCH + kq);
    }
    for (int idx = threadIdx.x; idx < kGTile * qg; idx += nthreads) {
      const int p = idx / qg, kq = (idx - p * qg) * 4;
      const int py = p / TW, px = p - py * TW;
      const int gy = y0 + py, gx = x0 + px, c = co0 + kq;
      const bool inside = gy < a.H && gx < a.W;
      stage_quad<NS>(gb + ((int64_t)gy * a.W + gx) * a.ldg + c, inside, c, a.Cout, a.vecg, gimg, kGImg, p * PITCH + kq);
    }
    __syncthreads();
    // k-step ks = tile rows 2 ks, 2 ks + 1: lane group mh holds pixels 8 mh .. 8 mh + 7 of the 32
    bf16x8 fg[4][NS];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int s = 0; s < NS; ++s)
        fg[ks][s] = frag_pixels(gimg + s * kGImg, (2 * ks + (mh >> 1)) * TW + 8 * (mh & 1), 16 * tco, lane);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        bf16x8 fx[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s)
          fx[s] = frag_pixels(ximg + s * kXImg, (2 * ks + (mh >> 1) + ky) * PW + 8 * (mh & 1) + kx, 16 * tci, lane);
        // terms (g image t - i) . (x image i), from the smallest to hi . hi
#pragma unroll
        for (int t = NS - 1; t >= 0; --t)
#pragma unroll
          for (int i = 0; i <= t; ++i)
            acc[tap] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fg[ks][t - i], fx[i], acc[tap], 0, 0, 0);
      }
    }
    __syncthreads();                                         // every wave is done reading this tile's images
  }

  // D register t of lane (mi, mh): output channel 4 mh + t (A row), input channel mi (B column)
  float *dst = a.dst + (int64_t)blockIdx.x * a.count;
  const int ci = ci0 + 16 * tci + mi;
  if (ci >= a.Cin) return;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int co = co0 + 16 * tco + 4 * mh + t;
    if (co >= a.Cout) continue;
    // ConvTranspose2d: gWt[ci][co][a][b] = gWc[co][ci][2 - a][2 - b]
    float *d = dst + (a.transposed ? ((int64_t)ci * a.Cout + co) : ((int64_t)co * a.Cin + ci)) * 9;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) d[a.transposed ? 8 - tap : tap] = acc[tap][t];
  }
}

// How a weight gradient is cut into blocks.  Channel tiles per block: up to 2 x 2 tiles of 16 x 16 (one wave each).
// Pixel chunks: as many as bring the grid to about 1024 blocks, never more than there are pixel tiles -- many at high
// resolution (few channel groups, many pixels), one or two at low resolution.
struct WgradPlan { int nco, nci; int64_t groups, tiles, tpc, chunks; };
inline WgradPlan wgrad_plan(int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout) {
  WgradPlan p;
  const int64_t jco = (Cout + 15) / 16, jci = (Cin + 15) / 16;
  p.nco = jco >= 2 ? 2 : 1;
  p.nci = jci >= 2 ? 2 : 1;
  p.groups = ((jco + p.nco - 1) / p.nco) * ((jci + p.nci - 1) / p.nci);
  p.tiles = B * ((H + TH - 1) / TH) * ((W + TW - 1) / TW);
  int64_t want = (1024 + p.groups - 1) / p.groups;
  if (want > p.tiles) want = p.tiles;
  if (want < 1) want = 1;
  p.tpc = (p.tiles + want - 1) / want;
  p.chunks = (p.tiles + p.tpc - 1) / p.tpc;
  return p;
}

inline bool wgrad_sizes_ok(int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout) {
  return B >= 0 && H >= 0 && W >= 0 && Cin >= 1 && Cin <= kMaxC && Cout >= 1 && Cout <= kMaxC;
}
// 0: no slabs (one chunk or an empty call); -1: out of range
inline int64_t wgrad_workspace(int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t ldg, int64_t ldx) {
  if (H >= (1 << 30) || W >= (1 << 30) || (H > 0 && W > 0 && B > INT64_MAX / H / W)) return -1;
  const int64_t rows = B * H * W;
  if (!fits(rows, ldg) || !fits(rows, ldx)) return -1;
  if (rows == 0) return 0;
  const WgradPlan p = wgrad_plan(B, H, W, Cin, Cout);
  if (p.tiles >= (int64_t(1) << 31) || p.groups > 65535) return -1;
  if (p.chunks <= 1) return 0;
  const int64_t count = 9 * Cin * Cout;
  if (p.chunks > (k4GiB / 4 - 1) / count) return -1;         // the slabs would reach 4 GiB
  return p.chunks * count;
}

// ---- the adjoint of k_upsample2x: every input pixel sums the output pixels that read it, ascending (oy, ox) ----
// output o reads inputs a = floor(o (n - 1) / d) and a + 1, d = 2 n - 1; input i is read by the o with a in {i - 1, i}:
// ceil((i - 1) d / (n - 1)) <= o <= ceil((i + 1) d / (n - 1)) - 1, clamped to [0, 2 n - 1]
__device__ inline void up_range(int i, int n, int &lo, int &hi) {
  if (n == 1) { lo = 0; hi = 1; return; }
  const int d = 2 * n - 1, m = n - 1;
  lo = i == 0 ? 0 : ((i - 1) * d + m - 1) / m;
  hi = ((i + 1) * d + m - 1) / m - 1;
  if (hi > 2 * n - 1) hi = 2 * n - 1;
}
// the weight with which output o reads input i: the same expressions as k_upsample2x's ly / lx
__device__ inline float up_weight(int o, int i, int n) {
  const int d = 2 * n - 1;
  const int a = o * (n - 1) / d;
  const float l = (float)(o * (n - 1) - a * d) / (float)d;
  const int b = a + (a < n - 1);
  float w = 0.0f;
  if (a == i) w = 1.0f - l;
  if (b == i) w = a == i ? w + l : l;
  return w;
}

__global__ __launch_bounds__(256) void k_upsample2x_bwd(const float *__restrict__ g, const float *__restrict__ mask,
                                                       float *__restrict__ out, int64_t total, int32_t Hin,
                                                       int32_t Win, int32_t C, int64_t ldg, int64_t ldm, int64_t ldo) {
  const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  const int64_t pix = idx / C;
  const int ix = (int)(pix % Win), iy = (int)((pix / Win) % Hin);
  const int64_t b = pix / ((int64_t)Win * Hin);
  const int Wo = 2 * Win;
  int ylo, yhi, xlo, xhi;
  up_range(iy, Hin, ylo, yhi);
  up_range(ix, Win, xlo, xhi);
  const int64_t base = b * 4 * Hin * Win;
  float s = 0.0f;
  for (int oy = ylo; oy <= yhi; ++oy) {
    const float wy = up_weight(oy, iy, Hin);
    for (int ox = xlo; ox <= xhi; ++ox) {
      const float wx = up_weight(ox, ix, Win);
      const int64_t o = base + (int64_t)oy * Wo + ox;
      float v = g[o * ldg + c];
      if (mask && !(mask[o * ldm + c] > 0.0f)) v = 0.0f;
      s = s + wy * (wx * v);
    }
  }
  out[pix * ldo + c] = s;
}

// ---- ReLU + BatchNorm backward ----
// stage 1 / stage 2 as k_stats_partial / k_stats_finish: sums of g_z and of g_z xhat in fp64, g_z = g_y [y > 0],
// xhat = (pre - mean) rstd
__global__ __launch_bounds__(256) void k_bn_bwd_partial(const float *__restrict__ gy, const float *__restrict__ y,
                                                       const float *__restrict__ pre, const double *__restrict__ mean,
                                                       const double *__restrict__ rstd, double *__restrict__ part,
                                                       int64_t rows, int32_t C, int64_t ldg, int64_t ldy, int64_t ldp,
                                                       int64_t chunk_rows) {
  __shared__ double sh[2][kStatLanes][64];
  const int c = blockIdx.y * 64 + threadIdx.x, gl = threadIdx.y;
  const int64_t lo = blockIdx.x * chunk_rows, hi = lo + chunk_rows < rows ? lo + chunk_rows : rows;
  double s = 0.0, q = 0.0;
  if (c < C) {
    const double m = mean[c], r = rstd[c];
    for (int64_t row = lo + gl; row < hi; row += kStatLanes) {
      const double gz = y[row * ldy + c] > 0.0f ? (double)gy[row * ldg + c] : 0.0;
      s = s + gz;
      q = q + gz * (((double)pre[row * ldp + c] - m) * r);
    }
  }
  sh[0][gl][threadIdx.x] = s;
  sh[1][gl][threadIdx.x] = q;
  __syncthreads();
  if (gl == 0 && c < C) {
    s = sh[0][0][threadIdx.x]; q = sh[1][0][threadIdx.x];
    for (int k = 1; k < kStatLanes; ++k) { s = s + sh[0][k][threadIdx.x]; q = q + sh[1][k][threadIdx.x]; }
    part[((int64_t)blockIdx.x * 2) * C + c] = s;
    part[((int64_t)blockIdx.x * 2 + 1) * C + c] = q;
  }
}

// sums[0][c] = g_beta, sums[1][c] = g_gamma: the chunks in order
__global__ __launch_bounds__(256) void k_bn_bwd_finish(const double *__restrict__ part, double *__restrict__ sums,
                                                      int32_t C, int64_t chunks) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s = 0.0, q = 0.0;
  for (int64_t k = 0; k < chunks; ++k) { s = s + part[(k * 2) * C + c]; q = q + part[(k * 2 + 1) * C + c]; }
  sums[c] = s;
  sums[C + c] = q;
}

// train: g_p = gamma r (g_z - g_beta / n - xhat g_gamma / n); eval: g_p = gamma r g_z.  fp32.
__global__ __launch_bounds__(256) void k_bn_bwd_apply(const float *__restrict__ gy, const float *__restrict__ y,
                                                     const float *__restrict__ pre, const float *__restrict__ gamma,
                                                     const double *__restrict__ mean, const double *__restrict__ rstd,
                                                     const double *__restrict__ sums, float *__restrict__ out,
                                                     int64_t total, int64_t rows, int32_t C, int64_t ldg, int64_t ldy,
                                                     int64_t ldp, int64_t ldo, int32_t train) {
  const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  const int64_t row = idx / C;
  const float r = (float)rstd[c];
  const float gz = y[row * ldy + c] > 0.0f ? gy[row * ldg + c] : 0.0f;
  float v = gz;
  if (train) {
    const float xh = (pre[row * ldp + c] - (float)mean[c]) * r;
    const float gb = (float)(sums[c] / (double)rows), gg = (float)(sums[C + c] / (double)rows);
    v = gz - gb - xh * gg;
  }
  out[row * ldo + c] = (gamma[c] * r) * v;
}

// out[b, y, x, c] = g_p[b, y / 2, x / 2, c] where (y & 1, x & 1) is the window's winner, else 0 (also in the last odd
// row / column, which the floor rule left out of every window)
__global__ __launch_bounds__(256) void k_unpool2x2(const float *__restrict__ gp, const uint8_t *__restrict__ argmax,
                                                  float *__restrict__ out, int64_t total, int32_t H, int32_t W,
                                                  int32_t C, int64_t ldg, int64_t ldo) {
  const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  const int64_t pix = idx / C;
  const int x = (int)(pix % W), y = (int)((pix / W) % H);
  const int64_t b = pix / ((int64_t)W * H);
  const int Hp = H >> 1, Wp = W >> 1, py = y >> 1, px = x >> 1;
  float v = 0.0f;
  if (py < Hp && px < Wp) {
    const int64_t o = (b * Hp + py) * Wp + px;
    if (argmax[o * C + c] == (uint8_t)((y & 1) * 2 + (x & 1))) v = gp[o * ldg + c];
  }
  out[pix * ldo + c] = v;
}

}  // namespace

extern "C" int gwen_conv3x3_grad_weight_plan(int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                                             int *channel_tiles, int64_t *pixel_chunks) {
  if (!wgrad_sizes_ok(B, H, W, Cin, Cout) || B < 1 || H < 1 || W < 1 || !channel_tiles || !pixel_chunks)
    return GWEN_EINVAL;
  if (H >= (1 << 30) || W >= (1 << 30) || B > INT64_MAX / H / W) return GWEN_ERANGE;
  const WgradPlan p = wgrad_plan(B, H, W, Cin, Cout);
  *channel_tiles = p.nco * p.nci;
  *pixel_chunks = p.chunks;
  return GWEN_OK;
}

extern "C" int64_t gwen_conv3x3_grad_weight_workspace_floats(int64_t B, int64_t H, int64_t W, int64_t Cin,
                                                             int64_t Cout) {
  if (!wgrad_sizes_ok(B, H, W, Cin, Cout)) return 0;
  return wgrad_workspace(B, H, W, Cin, Cout, Cout, Cin);
}

extern "C" int gwen_conv3x3_grad_weight_f32(const float *g, const float *x, float *gw, int64_t B, int64_t H, int64_t W,
                                            int64_t Cin, int64_t Cout, int64_t ldg, int64_t ldx, int transposed,
                                            int contract, float *workspace, int64_t workspace_floats,
                                            gwen_stream_t stream) {
  if (!wgrad_sizes_ok(B, H, W, Cin, Cout) || ldg < Cout || ldx < Cin || transposed < 0 || transposed > 1 ||
      !split_contract(contract))
    return GWEN_EINVAL;
  const int64_t need = wgrad_workspace(B, H, W, Cin, Cout, ldg, ldx);
  if (need < 0) return GWEN_ERANGE;
  if (!gw || !gwen_aligned(gw, 4)) return GWEN_EINVAL;
  hipStream_t st = gwen_stream(stream);
  const int64_t count = 9 * Cin * Cout;
  if (B * H * W == 0) {                                      // an empty sum
    GWEN_HIP_CHECK(hipMemsetAsync(gw, 0, (size_t)count * 4, st));
    return GWEN_OK;
  }
  if (!g || !x || g == gw || x == gw || !gwen_aligned(g, 4) || !gwen_aligned(x, 4)) return GWEN_EINVAL;
  if (need > 0 && (!workspace || workspace_floats < need || !gwen_aligned(workspace, 4))) return GWEN_ENOSPACE;
  const WgradPlan p = wgrad_plan(B, H, W, Cin, Cout);
  WgradArgs a;
  a.g = g; a.x = x; a.dst = p.chunks > 1 ? workspace : gw;
  a.H = (int32_t)H; a.W = (int32_t)W; a.Cin = (int32_t)Cin; a.Cout = (int32_t)Cout;
  a.tiles_x = (int32_t)((W + TW - 1) / TW); a.tiles_y = (int32_t)((H + TH - 1) / TH);
  a.nci = p.nci; a.gci = (int32_t)(((Cin + 15) / 16 + p.nci - 1) / p.nci);
  a.transposed = transposed;
  a.vecg = Cout % 4 == 0 && ldg % 4 == 0 && gwen_aligned(g, 16);
  a.vecx = Cin % 4 == 0 && ldx % 4 == 0 && gwen_aligned(x, 16);
  a.ldg = ldg; a.ldx = ldx; a.tiles = p.tiles; a.tpc = p.tpc; a.count = count;
  const dim3 grid((unsigned)p.chunks, (unsigned)p.groups);
  const unsigned threads = 64u * p.nco * p.nci;
  if (gwen_dense_contract(contract) == GWEN_CONTRACT_BF16X6) k_conv3x3_wgrad<3><<<grid, threads, 0, st>>>(a);
  else k_conv3x3_wgrad<2><<<grid, threads, 0, st>>>(a);
  GWEN_LAUNCH_CHECK();
  if (p.chunks <= 1) return GWEN_OK;
  const gwen_reduce_task task{workspace, gw, count, p.chunks};
  return gwen_reduce_chunks_batched(&task, 1, stream);
}

extern "C" int gwen_upsample2x_backward_f32(const float *g, const float *mask, float *out, int64_t B, int64_t Hin,
                                            int64_t Win, int64_t C, int64_t ldg, int64_t ldm, int64_t ldo,
                                            gwen_stream_t stream) {
  if (B < 0 || Hin < 0 || Win < 0 || C < 1 || C > kMaxC || ldg < C || ldo < C || (mask && ldm < C)) return GWEN_EINVAL;
  if (Hin >= (1 << 14) || Win >= (1 << 14) || (Hin > 0 && Win > 0 && B > INT64_MAX / 4 / Hin / Win)) return GWEN_ERANGE;
  const int64_t rows_in = B * Hin * Win;
  if (!fits(rows_in * 4, ldg) || !fits(rows_in, ldo) || (mask && !fits(rows_in * 4, ldm))) return GWEN_ERANGE;
  if (rows_in == 0) return GWEN_OK;
  if (!g || !out || g == out || mask == out || !gwen_aligned(g, 4) || !gwen_aligned(out, 4) ||
      (mask && !gwen_aligned(mask, 4)))
    return GWEN_EINVAL;
  const int64_t total = rows_in * C;
  k_upsample2x_bwd<<<(unsigned)((total + 255) / 256), 256, 0, gwen_stream(stream)>>>(
      g, mask, out, total, (int32_t)Hin, (int32_t)Win, (int32_t)C, ldg, mask ? ldm : 0, ldo);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

extern "C" int gwen_norm_relu_backward_f32(const float *g_y, const float *y, const float *pre, const float *weight,
                                           const double *mean, const double *rstd, float *g_pre, double *sums,
                                           int64_t rows, int64_t C, int64_t ldg, int64_t ldy, int64_t ldp, int64_t ldo,
                                           int train, void *workspace, int64_t workspace_bytes, gwen_stream_t stream) {
  if (rows < 1 || C < 1 || C > kMaxC || ldg < C || ldy < C || ldp < C || ldo < C || train < 0 || train > 1)
    return GWEN_EINVAL;
  if (!fits(rows, ldg) || !fits(rows, ldy) || !fits(rows, ldp) || !fits(rows, ldo)) return GWEN_ERANGE;
  if (!g_y || !y || !pre || !weight || !mean || !rstd || !g_pre || !sums || !workspace || g_pre == y || g_pre == pre || g_pre == g_y ||
      !gwen_aligned(g_y, 4) || !gwen_aligned(y, 4) || !gwen_aligned(pre, 4) || !gwen_aligned(weight, 4) ||
      !gwen_aligned(g_pre, 4) || !gwen_aligned(mean, 8) || !gwen_aligned(rstd, 8) || !gwen_aligned(sums, 8) ||
      !gwen_aligned(workspace, 8))
    return GWEN_EINVAL;
  const int64_t chunks = stat_chunks(rows);
  if (workspace_bytes < chunks * 2 * C * (int64_t)sizeof(double)) return GWEN_ENOSPACE;
  hipStream_t st = gwen_stream(stream);
  double *part = static_cast<double *>(workspace);
  k_bn_bwd_partial<<<dim3((unsigned)chunks, (unsigned)((C + 63) / 64)), dim3(64, kStatLanes), 0, st>>>(
      g_y, y, pre, mean, rstd, part, rows, (int32_t)C, ldg, ldy, ldp, stat_chunk_rows(rows));
  GWEN_LAUNCH_CHECK();
  k_bn_bwd_finish<<<(unsigned)((C + 255) / 256), 256, 0, st>>>(part, sums, (int32_t)C, chunks);
  GWEN_LAUNCH_CHECK();
  const int64_t total = rows * C;
  k_bn_bwd_apply<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(g_y, y, pre, weight, mean, rstd, sums, g_pre, total,
                                                                 rows, (int32_t)C, ldg, ldy, ldp, ldo, train);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

extern "C" int gwen_unpool2x2_f32(const float *g_p, const uint8_t *argmax, float *out, int64_t B, int64_t H, int64_t W,
                                  int64_t C, int64_t ldg, int64_t ldo, gwen_stream_t stream) {
  if (B < 0 || H < 0 || W < 0 || C < 1 || C > kMaxC || ldg < C || ldo < C) return GWEN_EINVAL;
  if (H >= (1 << 30) || W >= (1 << 30) || (H > 0 && W > 0 && B > INT64_MAX / H / W)) return GWEN_ERANGE;
  const int64_t rows = B * H * W, rows_p = B * (H / 2) * (W / 2);
  if (!fits(rows, ldo) || !fits(rows_p, ldg)) return GWEN_ERANGE;
  if (rows == 0) return GWEN_OK;
  if (!out || !gwen_aligned(out, 4) || (rows_p > 0 && (!g_p || !argmax || g_p == out || !gwen_aligned(g_p, 4))))
    return GWEN_EINVAL;
  const int64_t total = rows * C;
  if ((total + 255) / 256 > 0x7fffffffLL) return GWEN_ERANGE;
  k_unpool2x2<<<(unsigned)((total + 255) / 256), 256, 0, gwen_stream(stream)>>>(g_p, argmax, out, total, (int32_t)H,
                                                                              (int32_t)W, (int32_t)C, ldg, ldo);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}
