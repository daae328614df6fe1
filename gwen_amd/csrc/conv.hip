// U-Net kernels (gwen_amd.models_cnn; the reference's second model family, its src/gwen/models_cnn.py):
//   gwen_conv3x3_f32        3x3 / stride 1 / padding 1 convolution as an implicit GEMM on the split contractions of
//                           split.h, with bias, per-channel affine, ReLU and a 2x2 / stride 2 max-pool in the epilogue;
//   gwen_conv3x3_argmax_f32 the same launch that also keeps the pool's argmax and the pooled value (the backward's);
//   gwen_conv3x3_pack_f32   Conv2d or ConvTranspose2d weights -> the B fragments the conv kernel reads, tap by tap;
//   gwen_upsample2x_f32     bilinear x2, align_corners = True, with the same affine + ReLU;
//   gwen_channel_stats_f64  per-channel mean / biased variance in fp64 (train-mode BatchNorm);
//   gwen_affine_relu_f32    y = max(0, x s[c] + t[c]) in place.
// Activations are channels-last fp32: [B, H, W, C] is a row matrix [B H W, C] with a row pitch ld >= C.
//
// The conv kernel.  v_mfma_f32_16x16x32_bf16 with the PIXELS as the A rows and the output channels as the B columns:
// lane (mi, mh) = (lane & 15, lane >> 4) holds A[pixel mi][k = 8 mh .. +8) and B[k = 8 mh .. +8)[channel mi]; D register t
// is D[pixel 4 mh + t][channel mi].  A block (4 waves) owns 8 x 16 output pixels of one image and NCT <= 4 tiles of 16
// output channels; wave w owns tile rows 2 w and 2 w + 1 (one 16-pixel A tile each).  Per 32-channel chunk of Cin the
// block stages the 10 x 18 halo patch in LDS, already cut into the NS bf16 images (once, not once per tap; pixel pitch
// 48 bf16 = 96 B: the 16-byte fragment reads of a lane group fall on 16 different slots), then runs the 9 taps: the A
// fragment of tap (ky, kx) is the patch read at pixel (row + ky, mi + kx), the B fragment one 1-KiB run of the packed
// image.  Lanes beyond Cin and pixels outside the image are written as zeros by a select -- memory there is never read.
// The 2x2 pool is lane-local: its window is rows 2 w, 2 w + 1 (both of this wave) x pixels 4 mh + {0, 1} or {2, 3}.
// One block computes an output element, k ascending (chunk outer, tap inner) -- or, where an image alone gives too few
// blocks to fill the chip, a fixed number of blocks one slice of Cin each, their raw sums added in slice order by
// k_conv3x3_finish (conv_plan below; the cut depends on one image's shape only): bitwise reproducible, and the same
// bits for an image whatever the batch around it.  No atomics; element offsets are 64-bit.
#include "conv_common.h"

namespace {

struct ConvArgs {
  const float *x;
  const __bf16 *P;
  const float *bias, *scale, *shift;
  float *out;
  int32_t H, W, Cin, Cout, tiles_x, tiles_y, jn, flags;
  int64_t ldx, ldo;
  float *part;           // split over Cin: slice z = blockIdx.z writes its raw sums to part[z][B H W][Cout]; else NULL
  int32_t cpz;           // 32-channel chunks per slice
  int64_t rows;          // B H W
  uint8_t *argmax;       // gwen_conv3x3_argmax_f32: the pool's winner per output element [B, H/2, W/2, Cout], and
  float *pre;            // (optional) the pooled value + bias before affine and ReLU, pitch ldp
  int64_t ldp;
};

__device__ inline float max_nan(float a, float b) { return (a > b || a != a) ? a : b; }     // NaN wins, as torch's pool
// max_nan's comparison with the index carried along, in window order (0,0) (0,1) (1,0) (1,1): the first strictly
// largest value wins, a NaN replaces whatever came before it (torch's max_pool2d rule)
__device__ inline int argmax_nan(float v0, float v1, float v2, float v3) {
  float m = v0;
  int i = 0;
  if (v1 > m || v1 != v1) { m = v1; i = 1; }
  if (v2 > m || v2 != v2) { m = v2; i = 2; }
  if (v3 > m || v3 != v3) { m = v3; i = 3; }
  return i;
}

template <int NS, int NCT, bool VEC, bool AM = false>
__global__ __launch_bounds__(kThreads) void k_conv3x3(const ConvArgs a) {
  __shared__ __attribute__((aligned(16))) __bf16 img[NS * kPatch * PITCH];
  constexpr int kImg = kPatch * PITCH;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, mi = lane & 15, mh = lane >> 4;
  const int tx = blockIdx.x % a.tiles_x, ty = (blockIdx.x / a.tiles_x) % a.tiles_y;
  const int64_t b = blockIdx.x / (a.tiles_x * a.tiles_y);
  const int y0 = ty * TH, x0 = tx * TW, j0 = blockIdx.y * NCT;
  const float *xb = a.x + b * a.H * a.W * a.ldx;

  f32x4 acc[2][NCT];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int kcn = (a.Cin + CK - 1) / CK;
  const int kc_lo = blockIdx.z * a.cpz, kc_hi = kc_lo + a.cpz < kcn ? kc_lo + a.cpz : kcn;
  for (int kc = kc_lo; kc < kc_hi; ++kc) {
    // the halo patch of this chunk: (pixel, channel quad) items, split and parked as bf16x4
    for (int idx = threadIdx.x; idx < kPatch * (CK / 4); idx += kThreads) {
      const int p = idx >> 3, kq = (idx & 7) * 4;
      const int py = p / PW, px = p - py * PW;
      const int gy = y0 - 1 + py, gx = x0 - 1 + px, c = kc * CK + kq;
      float f4[4] = {0.f, 0.f, 0.f, 0.f};
      if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W && c < a.Cin) {
        const float *src = xb + ((int64_t)gy * a.W + gx) * a.ldx + c;
        if constexpr (VEC) {                                 // Cin % 4 == 0: a quad is inside or outside as a whole
          const float4_t v = *reinterpret_cast<const float4_t *>(src);
          f4[0] = v[0]; f4[1] = v[1]; f4[2] = v[2]; f4[3] = v[3];
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (c + e < a.Cin) f4[e] = src[e];
        }
      }
      bf16x4 im[NS];
      gwen::split_images<4, NS>(f4, im);
#pragma unroll
      for (int s = 0; s < NS; ++s) *reinterpret_cast<bf16x4 *>(img + s * kImg + p * PITCH + kq) = im[s];
    }
    __syncthreads();
    // (a rolled loop over the taps with one running fragment pointer: unrolled, the 9 x NCT fragment addresses are
    // kept in scalar registers and spill)
    const __bf16 *pt = a.P + ((int64_t)kc * 9 * a.jn + j0) * NS * kFrag + lane * 8;
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap, pt += (int64_t)a.jn * NS * kFrag) {
      const int ky = tap / 3, kx = tap - 3 * ky;
      bf16x8 fa[2][NS];
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        const int off = ((2 * wave + rt + ky) * PW + mi + kx) * PITCH + 8 * mh;
#pragma unroll
        for (int s = 0; s < NS; ++s) fa[rt][s] = *reinterpret_cast<const bf16x8 *>(img + s * kImg + off);
      }
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        if (j0 + ct >= a.jn) continue;                       // (block-uniform) no such column tile: nothing is read
        const __bf16 *pf = pt + ct * NS * kFrag;
        bf16x8 fb[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) fb[s] = *reinterpret_cast<const bf16x8 *>(pf + s * kFrag);
        // terms (x image t - i) . (W image i), from the smallest to hi . hi (K3's order)
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
          for (int t = NS - 1; t >= 0; --t)
#pragma unroll
            for (int i = 0; i <= t; ++i)
              acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[rt][t - i], fb[i], acc[rt][ct], 0, 0, 0);
      }
    }
    __syncthreads();                                         // every wave is done reading this chunk's patch
  }

  if (a.part) {                                              // a slice's raw sums; k_conv3x3_finish adds the slices in order
    float *slab = a.part + (int64_t)blockIdx.z * a.rows * a.Cout;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      const int c = (j0 + ct) * 16 + mi;
      if (j0 + ct >= a.jn || c >= a.Cout) continue;
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int y = y0 + 2 * wave + rt, x = x0 + 4 * mh + t;
          if (y < a.H && x < a.W) slab[((b * a.H + y) * a.W + x) * a.Cout + c] = acc[rt][ct][t];
        }
    }
    return;
  }
  const bool affine = a.flags & GWEN_CONV_AFFINE, relu = a.flags & GWEN_CONV_RELU, pool = a.flags & GWEN_CONV_POOL;
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    const int c = (j0 + ct) * 16 + mi;
    if (j0 + ct >= a.jn || c >= a.Cout) continue;
    const float bv = a.bias ? a.bias[c] : 0.0f;
    const float sc = affine ? a.scale[c] : 1.0f, sh = affine ? a.shift[c] : 0.0f;
    if (!pool) {
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int y = y0 + 2 * wave + rt, x = x0 + 4 * mh + t;
          if (y >= a.H || x >= a.W) continue;
          float v = acc[rt][ct][t] + bv;
          if (affine) v = v * sc + sh;
          if (relu) v = v < 0.0f ? 0.0f : v;
          a.out[((b * a.H + y) * a.W + x) * a.ldo + c] = v;
        }
    } else {                                                 // max first (the encoder's order), then bias: rounding is monotonic
      const int Hp = a.H >> 1, Wp = a.W >> 1, py = (y0 >> 1) + wave;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int px = (x0 >> 1) + 2 * mh + q;
        if (py >= Hp || px >= Wp) continue;
        float v = max_nan(max_nan(acc[0][ct][2 * q], acc[0][ct][2 * q + 1]),
                          max_nan(acc[1][ct][2 * q], acc[1][ct][2 * q + 1])) + bv;
        if constexpr (AM) {
          const int64_t o = (b * Hp + py) * Wp + px;
          a.argmax[o * a.Cout + c] = (uint8_t)argmax_nan(acc[0][ct][2 * q], acc[0][ct][2 * q + 1], acc[1][ct][2 * q],
                                                         acc[1][ct][2 * q + 1]);
          if (a.pre) a.pre[o * a.ldp + c] = v;
        }
        if (affine) v = v * sc + sh;
        if (relu) v = v < 0.0f ? 0.0f : v;
        a.out[((b * Hp + py) * Wp + px) * a.ldo + c] = v;
      }
    }
  }
}

// out = epilogue(sum over the slices z, ascending, of part[z]): the pool's four pixels are summed each on its own first
__global__ __launch_bounds__(256) void k_conv3x3_finish(const float *__restrict__ part, const float *__restrict__ bias,
                                                       const float *__restrict__ scale, const float *__restrict__ shift,
                                                       float *__restrict__ out, int64_t total, int64_t rows, int32_t H,
                                                       int32_t W, int32_t Cout, int64_t ldo, int32_t nz, int32_t flags,
                                                       uint8_t *__restrict__ argmax, float *__restrict__ pre,
                                                       int64_t ldp) {
  const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const bool pool = flags & GWEN_CONV_POOL;
  const int Ho = pool ? H >> 1 : H, Wo = pool ? W >> 1 : W;
  const int c = (int)(idx % Cout);
  const int64_t pix = idx / Cout;
  const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho);
  const int64_t b = pix / ((int64_t)Wo * Ho);
  auto sum_at = [&](int y, int x) {
    const float *p = part + ((b * H + y) * W + x) * Cout + c;
    float s = 0.0f;
    for (int z = 0; z < nz; ++z) s = s + p[(int64_t)z * rows * Cout];
    return s;
  };
  float v;
  if (pool) {
    const float v0 = sum_at(2 * oy, 2 * ox), v1 = sum_at(2 * oy, 2 * ox + 1);
    const float v2 = sum_at(2 * oy + 1, 2 * ox), v3 = sum_at(2 * oy + 1, 2 * ox + 1);
    v = max_nan(max_nan(v0, v1), max_nan(v2, v3));
    if (argmax) argmax[pix * Cout + c] = (uint8_t)argmax_nan(v0, v1, v2, v3);
  } else {
    v = sum_at(oy, ox);
  }
  if (bias) v = v + bias[c];
  if (pre) pre[pix * ldp + c] = v;
  if (flags & GWEN_CONV_AFFINE) v = v * scale[c] + shift[c];
  if (flags & GWEN_CONV_RELU) v = v < 0.0f ? 0.0f : v;
  out[pix * ldo + c] = v;
}

// one block per (chunk kc, tap, column tile j), one thread per lane: the thread writes what that lane of the conv kernel
// holds as its B fragment -- [kc][tap][j][image s][lane][8] bf16, padded channels as zeros
template <int NS>
__global__ __launch_bounds__(64) void k_conv3x3_pack(const float *__restrict__ W, __bf16 *__restrict__ P, int32_t cin,
                                                    int32_t cout, int32_t jn, int32_t transposed) {
  const int lane = threadIdx.x, mi = lane & 15, mh = lane >> 4;
  const int j = blockIdx.x % jn, tap = (blockIdx.x / jn) % 9, kc = blockIdx.x / (9 * jn);
  const int co = j * 16 + mi;
  float wv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int ci = kc * CK + 8 * mh + i;
    float v = 0.0f;
    if (co < cout && ci < cin)      // ConvTranspose2d at stride 1, padding 1: Wc[co][ci][ky][kx] = Wt[ci][co][2 - ky][2 - kx]
      v = transposed ? W[((int64_t)ci * cout + co) * 9 + (8 - tap)] : W[((int64_t)co * cin + ci) * 9 + tap];
    wv[i] = v;
  }
  bf16x8 im[NS];
  gwen::split_images<8, NS>(wv, im);
#pragma unroll
  for (int s = 0; s < NS; ++s)
    *reinterpret_cast<bf16x8 *>(P + ((int64_t)blockIdx.x * NS + s) * kFrag + lane * 8) = im[s];
}

// out[b][oy][ox][c] = act(bilinear(in)[c] s[c] + t[c]); source position o (n - 1) / (2 n - 1) as an exact integer
// quotient and a correctly rounded fraction
__global__ __launch_bounds__(256) void k_upsample2x(const float *__restrict__ in, const float *__restrict__ scale,
                                                   const float *__restrict__ shift, float *__restrict__ out,
                                                   int64_t total, int32_t Hin, int32_t Win, int32_t C, int64_t ldi,
                                                   int64_t ldo, int32_t flags) {
  const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int Ho = 2 * Hin, Wo = 2 * Win;
  const int c = (int)(idx % C);
  const int64_t pix = idx / C;
  const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho);
  const int64_t b = pix / ((int64_t)Wo * Ho);
  const int dy = 2 * Hin - 1, dx = 2 * Win - 1;
  const int ya = oy * (Hin - 1) / dy, xa = ox * (Win - 1) / dx;
  const float ly = (float)(oy * (Hin - 1) - ya * dy) / (float)dy, lx = (float)(ox * (Win - 1) - xa * dx) / (float)dx;
  const int yb = ya + (ya < Hin - 1), xb = xa + (xa < Win - 1);
  const float *ib = in + b * Hin * Win * ldi + c;
  const float v00 = ib[((int64_t)ya * Win + xa) * ldi], v01 = ib[((int64_t)ya * Win + xb) * ldi];
  const float v10 = ib[((int64_t)yb * Win + xa) * ldi], v11 = ib[((int64_t)yb * Win + xb) * ldi];
  float v = (1.0f - ly) * ((1.0f - lx) * v00 + lx * v01) + ly * ((1.0f - lx) * v10 + lx * v11);
  if (flags & GWEN_CONV_AFFINE) v = v * scale[c] + shift[c];
  if (flags & GWEN_CONV_RELU) v = v < 0.0f ? 0.0f : v;
  out[pix * ldo + c] = v;
}

// stage 1: block (chunk of rows, 64 channels), thread (channel, row lane g of 4): rows g, g + 4, .. of the chunk in
// order, then the four lanes in order; stage 2: the chunks in order.  Sums of x and x^2 in fp64.
__global__ __launch_bounds__(256) void k_stats_partial(const float *__restrict__ x, double *__restrict__ part,
                                                      int64_t rows, int32_t C, int64_t ld, int64_t chunk_rows) {
  __shared__ double sh[2][kStatLanes][64];
  const int c = blockIdx.y * 64 + threadIdx.x, g = threadIdx.y;
  const int64_t lo = blockIdx.x * chunk_rows, hi = lo + chunk_rows < rows ? lo + chunk_rows : rows;
  double s = 0.0, q = 0.0;
  if (c < C)
    for (int64_t r = lo + g; r < hi; r += kStatLanes) {
      const double v = (double)x[r * ld + c];
      s = s + v;
      q = q + v * v;
    }
  sh[0][g][threadIdx.x] = s;
  sh[1][g][threadIdx.x] = q;
  __syncthreads();
  if (g == 0 && c < C) {
    s = sh[0][0][threadIdx.x]; q = sh[1][0][threadIdx.x];
    for (int k = 1; k < kStatLanes; ++k) { s = s + sh[0][k][threadIdx.x]; q = q + sh[1][k][threadIdx.x]; }
    part[((int64_t)blockIdx.x * 2) * C + c] = s;
    part[((int64_t)blockIdx.x * 2 + 1) * C + c] = q;
  }
}

__global__ __launch_bounds__(256) void k_stats_finish(const double *__restrict__ part, double *__restrict__ mean,
                                                     double *__restrict__ var, int64_t rows, int32_t C, int64_t chunks) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s = 0.0, q = 0.0;
  for (int64_t k = 0; k < chunks; ++k) { s = s + part[(k * 2) * C + c]; q = q + part[(k * 2 + 1) * C + c]; }
  const double m = s / (double)rows, v = q / (double)rows - m * m;
  mean[c] = m;
  var[c] = v < 0.0 ? 0.0 : v;
}

__global__ __launch_bounds__(256) void k_affine_relu(float *__restrict__ x, const float *__restrict__ scale,
                                                    const float *__restrict__ shift, int64_t total, int32_t C,
                                                    int64_t ld) {
  const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  float *p = x + (idx / C) * ld + c;
  const float v = *p * scale[c] + shift[c];
  *p = v < 0.0f ? 0.0f : v;
}

template <int NS, int NCT>
int launch_conv(const ConvArgs &a, bool vec, dim3 grid, hipStream_t st) {
  if (a.argmax && !a.part) {                                 // (a split call's argmax is k_conv3x3_finish's)
    if (vec) k_conv3x3<NS, NCT, true, true><<<grid, kThreads, 0, st>>>(a);
    else k_conv3x3<NS, NCT, false, true><<<grid, kThreads, 0, st>>>(a);
  } else if (vec) k_conv3x3<NS, NCT, true><<<grid, kThreads, 0, st>>>(a);
  else k_conv3x3<NS, NCT, false><<<grid, kThreads, 0, st>>>(a);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}
// How a layer is cut into blocks -- a function of ONE image's shape, never of the batch, so an image's bits do not
// depend on the items around it.  Column tiles per block: 4, fewer while an image gives under 256 blocks (low
// resolutions: many channels, few pixels); then the Cin chunks are split over up to 16 slices of at least 2 chunks
// whose raw sums k_conv3x3_finish adds in order (an 8 x 8 image at 1024 -> 512 channels: 8 blocks of 288 tap-steps
// become 256 of 36).
struct ConvPlan { int nct, nz, cpz; };
inline ConvPlan conv_plan(int64_t H, int64_t W, int64_t Cin, int64_t Cout, bool pool) {
  const int64_t tiles = (((pool ? W / 2 * 2 : W) + TW - 1) / TW) * (((pool ? H / 2 * 2 : H) + TH - 1) / TH);
  const int64_t jn = (Cout + 15) / 16, kcn = (Cin + CK - 1) / CK;
  int nct = jn >= 4 ? 4 : (int)jn;
  while (nct > 1 && tiles * ((jn + nct - 1) / nct) < 256) --nct;
  const int64_t blocks = tiles * ((jn + nct - 1) / nct);
  int64_t ks = 1;
  while (blocks * ks < 256 && ks < 16 && kcn / (ks * 2) >= 2) ks *= 2;
  const int cpz = (int)((kcn + ks - 1) / ks);
  return {nct, (int)((kcn + cpz - 1) / cpz), cpz};
}

template <int NS>
int launch_conv_nct(const ConvArgs &a, bool vec, int64_t tiles, int nct, int nz, hipStream_t st) {
  const dim3 grid((unsigned)tiles, (unsigned)((a.jn + nct - 1) / nct), (unsigned)nz);
  if (nct == 4) return launch_conv<NS, 4>(a, vec, grid, st);
  if (nct == 3) return launch_conv<NS, 3>(a, vec, grid, st);
  if (nct == 2) return launch_conv<NS, 2>(a, vec, grid, st);
  return launch_conv<NS, 1>(a, vec, grid, st);
}

}  // namespace

extern "C" int64_t gwen_conv3x3_pack_bytes(int64_t Cin, int64_t Cout, int contract) {
  if (Cin < 1 || Cin > kMaxC || Cout < 1 || Cout > kMaxC || !split_contract(contract)) return 0;
  const int ns = gwen::images_of(gwen_dense_contract(contract));
  return ((Cin + CK - 1) / CK) * 9 * ((Cout + 15) / 16) * ns * kFrag * 2;
}

extern "C" int gwen_conv3x3_pack_f32(const float *W, int64_t Cin, int64_t Cout, int transposed, int contract,
                                     void *packed, gwen_stream_t stream) {
  if (gwen_conv3x3_pack_bytes(Cin, Cout, contract) == 0 || transposed < 0 || transposed > 1) return GWEN_EINVAL;
  if (!W || !packed || !gwen_aligned(W, 4) || !gwen_aligned(packed, 16)) return GWEN_EINVAL;
  const int jn = (int)((Cout + 15) / 16);
  const unsigned blocks = (unsigned)(((Cin + CK - 1) / CK) * 9 * jn);
  __bf16 *P = static_cast<__bf16 *>(packed);
  hipStream_t st = gwen_stream(stream);
  if (gwen_dense_contract(contract) == GWEN_CONTRACT_BF16X6)
    k_conv3x3_pack<3><<<blocks, 64, 0, st>>>(W, P, (int32_t)Cin, (int32_t)Cout, jn, transposed);
  else
    k_conv3x3_pack<2><<<blocks, 64, 0, st>>>(W, P, (int32_t)Cin, (int32_t)Cout, jn, transposed);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

// The one place that says how a call runs: the plan, and the floats its slices need -- 0 without a split, -1 where the
// split's workspace [nz][B H W][Cout] would reach 4 GiB (the launcher refuses such a call: GWEN_ERANGE).  Sizes are
// already validated by the caller (B, H, W >= 1, B H W representable).
inline int64_t conv_workspace(const ConvPlan &p, int64_t B, int64_t H, int64_t W, int64_t Cout) {
  if (p.nz <= 1) return 0;
  const int64_t rows = B * H * W;
  if (rows > (k4GiB / 4) / p.nz || !fits(p.nz * rows, Cout)) return -1;
  return p.nz * rows * Cout;
}

extern "C" int gwen_conv3x3_plan(int64_t H, int64_t W, int64_t Cin, int64_t Cout, int flags, int *column_tiles,
                                 int *slices) {
  if (H < 1 || W < 1 || H >= (1 << 30) || W >= (1 << 30) || Cin < 1 || Cin > kMaxC || Cout < 1 || Cout > kMaxC ||
      flags < 0 || flags > (GWEN_CONV_AFFINE | GWEN_CONV_RELU | GWEN_CONV_POOL) || !column_tiles || !slices)
    return GWEN_EINVAL;
  const ConvPlan p = conv_plan(H, W, Cin, Cout, flags & GWEN_CONV_POOL);
  *column_tiles = p.nct;
  *slices = p.nz;
  return GWEN_OK;
}

extern "C" int64_t gwen_conv3x3_workspace_floats(int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int flags) {
  if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cin > kMaxC || Cout < 1 || Cout > kMaxC || flags < 0 ||
      flags > (GWEN_CONV_AFFINE | GWEN_CONV_RELU | GWEN_CONV_POOL))
    return 0;
  if (H >= (1 << 30) || W >= (1 << 30) || B > INT64_MAX / H / W) return -1;
  return conv_workspace(conv_plan(H, W, Cin, Cout, flags & GWEN_CONV_POOL), B, H, W, Cout);
}

namespace {
// gwen_conv3x3_f32 (argmax and pre NULL) and gwen_conv3x3_argmax_f32 (argmax given): one plan, one accumulation
int conv3x3_run(const float *x, const void *packed, const float *bias, const float *scale, const float *shift,
                float *out, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t ldx, int64_t ldo,
                int flags, int contract, float *workspace, int64_t workspace_floats, uint8_t *argmax, float *pre,
                int64_t ldp, bool want_argmax, gwen_stream_t stream) {
  if (B < 0 || H < 0 || W < 0 || gwen_conv3x3_pack_bytes(Cin, Cout, contract) == 0 || ldx < Cin || ldo < Cout)
    return GWEN_EINVAL;
  if (flags < 0 || flags > (GWEN_CONV_AFFINE | GWEN_CONV_RELU | GWEN_CONV_POOL)) return GWEN_EINVAL;
  if ((flags & GWEN_CONV_AFFINE) && (!scale || !shift)) return GWEN_EINVAL;
  if (want_argmax && (!(flags & GWEN_CONV_POOL) || ldp < Cout)) return GWEN_EINVAL;
  if (H >= (1 << 30) || W >= (1 << 30) || (H > 0 && W > 0 && B > INT64_MAX / H / W)) return GWEN_ERANGE;
  const bool pool = flags & GWEN_CONV_POOL;
  const int64_t Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
  if (!fits(B * H * W, ldx) || !fits(B * Ho * Wo, ldo) || (want_argmax && !fits(B * Ho * Wo, ldp))) return GWEN_ERANGE;
  if (B * Ho * Wo == 0) return GWEN_OK;
  // the plan decides the grid AND the workspace: a split (nz > 1) never runs without its slabs
  const ConvPlan p = conv_plan(H, W, Cin, Cout, pool);
  const int64_t need = conv_workspace(p, B, H, W, Cout);
  if (need < 0) return GWEN_ERANGE;
  // (HIP: grid.x * 256 threads < 2^32)
  const int64_t tiles = B * (((pool ? 2 * Wo : W) + TW - 1) / TW) * (((pool ? 2 * Ho : H) + TH - 1) / TH);
  if (tiles >= (1 << 24)) return GWEN_ERANGE;
  if (!x || !packed || !out || x == out || !gwen_aligned(x, 4) || !gwen_aligned(out, 4) || !gwen_aligned(packed, 16))
    return GWEN_EINVAL;
  if (want_argmax && (!argmax || (pre && (!gwen_aligned(pre, 4) || pre == out || pre == x)))) return GWEN_EINVAL;
  if (need > 0 && (!workspace || workspace_floats < need || !gwen_aligned(workspace, 4))) return GWEN_ENOSPACE;
  ConvArgs a;
  a.argmax = argmax; a.pre = pre; a.ldp = ldp;
  a.x = x; a.P = static_cast<const __bf16 *>(packed); a.bias = bias; a.scale = scale; a.shift = shift; a.out = out;
  a.H = (int32_t)H; a.W = (int32_t)W; a.Cin = (int32_t)Cin; a.Cout = (int32_t)Cout;
  // pooled: only the rows and columns some window covers (the floor rule's last odd row / column starts no tile)
  a.tiles_x = (int32_t)(((pool ? 2 * Wo : W) + TW - 1) / TW);
  a.tiles_y = (int32_t)(((pool ? 2 * Ho : H) + TH - 1) / TH);
  a.jn = (int32_t)((Cout + 15) / 16); a.flags = flags; a.ldx = ldx; a.ldo = ldo;
  const bool vec = Cin % 4 == 0 && ldx % 4 == 0 && gwen_aligned(x, 16);
  hipStream_t st = gwen_stream(stream);
  a.part = p.nz > 1 ? workspace : nullptr;
  a.cpz = p.cpz;
  a.rows = B * H * W;
  const int rc = gwen_dense_contract(contract) == GWEN_CONTRACT_BF16X6 ? launch_conv_nct<3>(a, vec, tiles, p.nct, p.nz, st)
                                                                        : launch_conv_nct<2>(a, vec, tiles, p.nct, p.nz, st);
  if (rc != GWEN_OK || p.nz <= 1) return rc;
  const int64_t total = B * Ho * Wo * Cout;
  k_conv3x3_finish<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(workspace, bias, scale, shift, out, total, a.rows,
                                                                   (int32_t)H, (int32_t)W, (int32_t)Cout, ldo, p.nz, flags,
                                                                   argmax, pre, ldp);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}
}  // namespace

extern "C" int gwen_conv3x3_f32(const float *x, const void *packed, const float *bias, const float *scale,
                                const float *shift, float *out, int64_t B, int64_t H, int64_t W, int64_t Cin,
                                int64_t Cout, int64_t ldx, int64_t ldo, int flags, int contract, float *workspace,
                                int64_t workspace_floats, gwen_stream_t stream) {
  return conv3x3_run(x, packed, bias, scale, shift, out, B, H, W, Cin, Cout, ldx, ldo, flags, contract, workspace,
                     workspace_floats, nullptr, nullptr, Cout, false, stream);
}

extern "C" int gwen_conv3x3_argmax_f32(const float *x, const void *packed, const float *bias, const float *scale,
                                       const float *shift, float *out, int64_t B, int64_t H, int64_t W, int64_t Cin,
                                       int64_t Cout, int64_t ldx, int64_t ldo, int flags, int contract,
                                       float *workspace, int64_t workspace_floats, uint8_t *argmax, float *pre,
                                       int64_t ldp, gwen_stream_t stream) {
  return conv3x3_run(x, packed, bias, scale, shift, out, B, H, W, Cin, Cout, ldx, ldo, flags, contract, workspace,
                     workspace_floats, argmax, pre, pre ? ldp : Cout, true, stream);
}

extern "C" int gwen_upsample2x_f32(const float *x, const float *scale, const float *shift, float *out, int64_t B,
                                   int64_t Hin, int64_t Win, int64_t C, int64_t ldx, int64_t ldo, int flags,
                                   gwen_stream_t stream) {
  if (B < 0 || Hin < 0 || Win < 0 || C < 1 || C > kMaxC || ldx < C || ldo < C) return GWEN_EINVAL;
  if (flags < 0 || flags > (GWEN_CONV_AFFINE | GWEN_CONV_RELU)) return GWEN_EINVAL;
  if ((flags & GWEN_CONV_AFFINE) && (!scale || !shift)) return GWEN_EINVAL;
  if (Hin >= (1 << 14) || Win >= (1 << 14) || (Hin > 0 && Win > 0 && B > INT64_MAX / 4 / Hin / Win)) return GWEN_ERANGE;
  const int64_t rows_out = B * Hin * Win * 4;
  if (!fits(rows_out, ldo) || !fits(rows_out, ldx)) return GWEN_ERANGE;
  if (rows_out == 0) return GWEN_OK;
  if (!x || !out || x == out || !gwen_aligned(x, 4) || !gwen_aligned(out, 4)) return GWEN_EINVAL;
  const int64_t total = rows_out * C;
  k_upsample2x<<<(unsigned)((total + 255) / 256), 256, 0, gwen_stream(stream)>>>(
      x, scale, shift, out, total, (int32_t)Hin, (int32_t)Win, (int32_t)C, ldx, ldo, flags);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

extern "C" int64_t gwen_channel_stats_workspace_bytes(int64_t rows, int64_t C) {
  if (rows < 1 || C < 1 || C > kMaxC) return 0;
  return stat_chunks(rows) * 2 * C * (int64_t)sizeof(double);
}

extern "C" int gwen_channel_stats_f64(const float *x, int64_t rows, int64_t C, int64_t ld, double *mean, double *var,
                                      void *workspace, int64_t workspace_bytes, gwen_stream_t stream) {
  if (rows < 1 || C < 1 || C > kMaxC || ld < C) return GWEN_EINVAL;
  if (!fits(rows, ld)) return GWEN_ERANGE;
  if (!x || !mean || !var || !workspace || !gwen_aligned(x, 4) || !gwen_aligned(mean, 8) || !gwen_aligned(var, 8) ||
      !gwen_aligned(workspace, 8))
    return GWEN_EINVAL;
  if (workspace_bytes < gwen_channel_stats_workspace_bytes(rows, C)) return GWEN_ENOSPACE;
  const int64_t chunks = stat_chunks(rows);
  hipStream_t st = gwen_stream(stream);
  double *part = static_cast<double *>(workspace);
  k_stats_partial<<<dim3((unsigned)chunks, (unsigned)((C + 63) / 64)), dim3(64, kStatLanes), 0, st>>>(
      x, part, rows, (int32_t)C, ld, stat_chunk_rows(rows));
  GWEN_LAUNCH_CHECK();
  k_stats_finish<<<(unsigned)((C + 255) / 256), 256, 0, st>>>(part, mean, var, rows, (int32_t)C, chunks);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

extern "C" int gwen_affine_relu_f32(float *x, const float *scale, const float *shift, int64_t rows, int64_t C,
                                    int64_t ld, gwen_stream_t stream) {
  if (rows < 0 || C < 1 || C > kMaxC || ld < C) return GWEN_EINVAL;
  if (!fits(rows, ld)) return GWEN_ERANGE;
  if (rows == 0) return GWEN_OK;
  if (!x || !scale || !shift || !gwen_aligned(x, 4)) return GWEN_EINVAL;
  const int64_t total = rows * C;
  k_affine_relu<<<(unsigned)((total + 255) / 256), 256, 0, gwen_stream(stream)>>>(x, scale, shift, total, (int32_t)C, ld);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}
