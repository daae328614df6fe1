// Spectral convolution of the spherical Fourier neural operator: a grouped GEMM over the degrees of a spherical
// harmonic expansion.  The coefficient rows of degree l are rows l^2 .. l^2 + 2l of [batch, T, C], T = (lmax + 1)^2,
// and every one of them is multiplied by that degree's own real matrix W[l] [Cin, Cout] (the spherical convolution
// theorem: a zonal filter multiplies every m of a degree by one factor, so the layer commutes with rotations).
//
//   k_spectral_conv    out[b, l^2 + j, :] = coef[b, l^2 + j, :] . W[l]   (or . W[l]^T with W stored [Cout, Cin]: the
//                      gradient in coef, no transposing copy)
//   k_spectral_grad_w  grad_W[l] = sum_b sum_j coef[b, l^2 + j, :]^T g[b, l^2 + j, :]
//
// Both contract on the split bf16 matrix cores (split.h): NS = 3 images is the fp32-class "bf16x6", NS = 2 "bf16x3";
// fp32 accumulators, ascending k.  W (the forward) and g^T (the weight gradient) are the MFMA A operand, the
// coefficient rows the B operand, so a lane ends with four consecutive output columns of one row: one 16-byte store.
//
// Forward geometry: grid (row-tile group, degree, column tile).  The batch is folded into the row axis -- a degree's
// rows are r -> (b = r / (2l + 1), j = r % (2l + 1)), batch * (2l + 1) of them -- so a block splits its W[l] panel
// [K, 64 or 32 columns] into images ONCE, parks them in LDS, and walks up to 16 64-row tiles against them; a tile may
// span several batch items and its tail is masked.  Blocks past a degree's last tile exit at once.  The rows never pass
// through LDS: a lane loads the 8 k-values a k-step of its own row straight from memory, a group of k-steps ahead of
// the MFMAs, and splits them in registers.
// An output element is the MFMA chain of its own row against W[l] in k order: it does not depend on which tile, wave
// or batch the row sits in, hence bitwise equal whatever the batch.
//
// Weight gradient: one block owns a 64 x 64 tile of grad_W[l] and walks the degree's rows in ascending r (b outer,
// j inner) in slabs of 32: no atomics, no split of the row axis, one fixed summation order.
#include "split.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRows = 64;             // rows of a forward tile: 4 waves x 16
constexpr int kPad = 8;               // bf16 elements between LDS rows: pitches stay 16-byte multiples, off the bank period
constexpr int kMaxTilesPerBlock = 16; // forward: row tiles a block walks against its staged panel, at most
constexpr int kSlab = 32;             // weight gradient: rows per k-step
constexpr int kSlabPitch = kSlab + kPad;

using gwen::bf16x4;
using gwen::bf16x8;

__host__ __device__ inline int round32(int k) { return (k + 31) & ~31; }

// global row of the local row r of degree l (m = 2l + 1 rows an item), batch item outer
__device__ inline int64_t global_row(int r, int m, int64_t T, int l) {
  const int b = r / m;
  return b * T + (int64_t)l * l + (r - b * m);
}

// NCT = 16-column tiles per block (4: 64 columns, K <= 256; 2: 32 columns, K <= 512 -- the panel's three images stay
// under 100 KB of LDS).  GK = k-steps of 32 a load group: a lane keeps two groups of its row in registers, the one being
// multiplied and the next one in flight (at 256 channels one block has a CU to itself, four waves: only the wave's own
// loads in flight hide the memory latency).  TW: W[l] stored [N, K] (read as its transpose) instead of [K, N].
// tpb = row tiles a block walks (the launcher's choice, at most kMaxTilesPerBlock).
template <int NS, int NCT, int GK, bool TW>
__global__ __launch_bounds__(kThreads) void k_spectral_conv(const float *__restrict__ coef, const float *__restrict__ W,
                                                            float *__restrict__ out, int batch, int lmax, int K, int N,
                                                            int tpb) {
  extern __shared__ __attribute__((aligned(16))) __bf16 panel[];     // [NS][NCT * 16][K32 + kPad]
  constexpr int BN = NCT * 16;
  constexpr int KMAX = GK < 8 ? GK * 32 : (NCT == 4 ? 256 : 512);     // the largest K this instantiation is launched with
  const int l = lmax - (int)blockIdx.y;                               // the longest degrees first
  const int m = 2 * l + 1;
  const int64_t nrows = (int64_t)batch * m;
  const int64_t ntiles = (nrows + kRows - 1) / kRows;
  const int64_t tile0 = (int64_t)blockIdx.x * tpb;
  if (tile0 >= ntiles) return;
  const int col0 = blockIdx.z * BN;
  const int K32 = round32(K), KP = K32 + kPad;
  const int img = BN * KP;
  const int64_t T = (int64_t)(lmax + 1) * (lmax + 1);
  const float *Wl = W + (int64_t)l * K * N;

  // a lane's share of the rows: the 8 k-values per k-step of row (wave, mi), in groups of GK k-steps.  The loads carry
  // no branch and no select (a select would make the wave wait for them at once): a masked lane reads row 0 of the
  // degree and is not stored; a k-step past K reads its own row's last 8 values again, which meet the panel's zeros
  // (a row that holds Inf or NaN is non-finite in every column either way).  The first group goes out before the panel
  // is staged.
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int mi = lane & 15, mh = lane >> 4;
  const int ksteps = K32 / 32, groups = (ksteps + GK - 1) / GK;
  const int ntl = (int)((tile0 + tpb < ntiles ? tile0 + tpb : ntiles) - tile0);
  auto load = [&](int t, int g, float4_t (&xr)[2 * GK]) {
    const int64_t r = (tile0 + t) * kRows + wave * 16 + mi;
    const float *p = coef + global_row(r < nrows ? (int)r : 0, m, T, l) * K;
#pragma unroll
    for (int q = 0; q < GK; ++q) {
      const int k = (g * GK + q) * 32 + 8 * mh;
      const int kk = k < K ? k : K - 8;
      xr[2 * q] = *reinterpret_cast<const float4_t *>(p + kk);
      xr[2 * q + 1] = *reinterpret_cast<const float4_t *>(p + kk + 4);
    }
  };
  int pt = 0, pg = 0;                                                 // the (tile, group) that is loaded next
  float4_t cur[2 * GK], nxt[2 * GK];
  load(pt, pg, cur);
  if (++pg == groups) { pg = 0; ++pt; }

  // ---- W[l]'s panel -> NS bf16 images [column][k], k in [K, K32) and columns past N zero.  Every load of a thread's
  // share goes out before the first split: the block pays the memory latency once, not once a loop trip. ----
  const int kquads = K32 / 4;
  if constexpr (TW) {
    constexpr int IT = BN * KMAX / 4 / kThreads;                       // float4 of a thread's share, at most 16
    float4_t v[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int idx = threadIdx.x + it * kThreads;
      const int n = idx / kquads, kq = idx - n * kquads;
      v[it] = float4_t{0.f, 0.f, 0.f, 0.f};
      if (n < BN && col0 + n < N && 4 * kq < K) v[it] = *reinterpret_cast<const float4_t *>(Wl + (int64_t)(col0 + n) * K + 4 * kq);
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int idx = threadIdx.x + it * kThreads;
      const int n = idx / kquads, kq = idx - n * kquads;
      if (n >= BN) break;
      const float f4[4] = {v[it][0], v[it][1], v[it][2], v[it][3]};
      bf16x4 im[NS];
      gwen::split_images<4, NS>(f4, im);
#pragma unroll
      for (int s = 0; s < NS; ++s) *reinterpret_cast<bf16x4 *>(panel + s * img + n * KP + 4 * kq) = im[s];
    }
  } else {
    constexpr int NQ = BN / 4;
    constexpr int IT = NQ * KMAX / 4 / kThreads;                       // 4 x 4 blocks of a thread's share, at most 4
    float4_t v[IT][4];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int idx = threadIdx.x + it * kThreads;
      const int kq = idx / NQ, n4 = (idx - kq * NQ) * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[it][e] = float4_t{0.f, 0.f, 0.f, 0.f};
        if (kq < kquads && col0 + n4 < N && 4 * kq < K)
          v[it][e] = *reinterpret_cast<const float4_t *>(Wl + (int64_t)(4 * kq + e) * N + col0 + n4);
      }
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int idx = threadIdx.x + it * kThreads;
      const int kq = idx / NQ, n4 = (idx - kq * NQ) * 4;
      if (kq >= kquads) break;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float f4[4] = {v[it][0][j], v[it][1][j], v[it][2][j], v[it][3][j]};
        bf16x4 im[NS];
        gwen::split_images<4, NS>(f4, im);
#pragma unroll
        for (int s = 0; s < NS; ++s) *reinterpret_cast<bf16x4 *>(panel + s * img + (n4 + j) * KP + 4 * kq) = im[s];
      }
    }
  }
  __syncthreads();

  // ---- the rows: GK k-steps of a lane's own row a load group, the next group in flight under this group's MFMAs.
  // Every column tile of the block is multiplied (the panel's columns past N are zero) so that the body of a k-step
  // has no branch: its twelve LDS reads go out together and the MFMAs of the four tiles interleave. ----
  for (int t = 0; t < ntl; ++t) {
    f32x4 acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int g = 0; g < groups; ++g) {
      const bool more = pt < ntl;
      if (more) {
        load(pt, pg, nxt);
        if (++pg == groups) { pg = 0; ++pt; }
      }
#pragma unroll
      for (int q = 0; q < GK; ++q) {
        const int ks = g * GK + q;
        if (ks >= ksteps) break;                                      // block-uniform
        const float x[8] = {cur[2 * q][0], cur[2 * q][1], cur[2 * q][2], cur[2 * q][3],
                            cur[2 * q + 1][0], cur[2 * q + 1][1], cur[2 * q + 1][2], cur[2 * q + 1][3]};
        bf16x8 b[NS];
        gwen::split_images<8, NS>(x, b);
        bf16x8 a[NCT][NS];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
          for (int s = 0; s < NS; ++s)
            a[ct][s] = *reinterpret_cast<const bf16x8 *>(panel + s * img + (ct * 16 + mi) * KP + ks * 32 + 8 * mh);
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[ct] = gwen::mma_split<8, NS>(a[ct], b, acc[ct]);
      }
      if (more) {
#pragma unroll
        for (int i = 0; i < 2 * GK; ++i) cur[i] = nxt[i];
      }
    }
    // D[column 4 mh + e][row mi]
    const int64_t r = (tile0 + t) * kRows + wave * 16 + mi;
    if (r < nrows) {
      float *dst = out + global_row((int)r, m, T, l) * N + col0 + 4 * mh;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
        if (col0 + ct * 16 < N) *reinterpret_cast<f32x4 *>(dst + ct * 16) = acc[ct];
    }
  }
}

// grad_W[l][i][o] = sum_r coef[r][i] g[r][o] over the degree's rows in ascending r.  Block tile: 64 i x 64 o; wave w
// owns the 16 i of tile w (the MFMA N axis) against four 16-wide o tiles (M).  A slab of 32 rows of both operands is
// turned [row][channel] -> [channel][row] on its way into LDS (threads 0 .. 127 coef, 128 .. 255 g: four rows x four
// channels each, split, one 8-byte store per channel and image); the next slab's loads are in flight under the MFMAs.
template <int NS>
__global__ __launch_bounds__(kThreads) void k_spectral_grad_w(const float *__restrict__ coef, const float *__restrict__ g,
                                                              float *__restrict__ grad_W, int batch, int lmax, int Cin,
                                                              int Cout) {
  __shared__ __attribute__((aligned(16))) __bf16 slab[2 * NS * 64 * kSlabPitch];     // [operand][NS][64 channels][32 rows + pad]
  constexpr int img = 64 * kSlabPitch;
  const int l = blockIdx.x;
  const int i0 = blockIdx.y * 64, o0 = blockIdx.z * 64;
  const int m = 2 * l + 1;
  const int64_t nrows = (int64_t)batch * m;
  const int64_t T = (int64_t)(lmax + 1) * (lmax + 1);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int mi = lane & 15, mh = lane >> 4;

  // this thread's share of a slab
  const int op = threadIdx.x >> 7, idx = threadIdx.x & 127;
  const int rq = idx >> 4, c4 = (idx & 15) * 4;
  const float *src = op ? g : coef;
  const int C = op ? Cout : Cin;
  const int c = (op ? o0 : i0) + c4;
  __bf16 *dst = slab + op * NS * img + c4 * kSlabPitch + 4 * rq;
  float4_t v[4];
  auto load = [&](int64_t r0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t r = r0 + 4 * rq + e;
      v[e] = float4_t{0.f, 0.f, 0.f, 0.f};
      if (r < nrows && c < C) v[e] = *reinterpret_cast<const float4_t *>(src + global_row((int)r, m, T, l) * C + c);
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float f4[4] = {v[0][j], v[1][j], v[2][j], v[3][j]};
      bf16x4 im[NS];
      gwen::split_images<4, NS>(f4, im);
#pragma unroll
      for (int s = 0; s < NS; ++s) *reinterpret_cast<bf16x4 *>(dst + s * img + j * kSlabPitch) = im[s];
    }
  };

  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  load(0);
  store();
  __syncthreads();
  for (int64_t r0 = 0; r0 < nrows; r0 += kSlab) {
    const bool more = r0 + kSlab < nrows;
    if (more) load(r0 + kSlab);
    bf16x8 b[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s)
      b[s] = *reinterpret_cast<const bf16x8 *>(slab + s * img + (wave * 16 + mi) * kSlabPitch + 8 * mh);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      bf16x8 a[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s)
        a[s] = *reinterpret_cast<const bf16x8 *>(slab + (NS + s) * img + (t * 16 + mi) * kSlabPitch + 8 * mh);
      acc[t] = gwen::mma_split<8, NS>(a, b, acc[t]);
    }
    __syncthreads();                     // every wave is done reading this slab
    if (more) {
      store();
      __syncthreads();
    }
  }
  // D[o = 4 mh + e][i = mi] of each tile
  const int i = i0 + wave * 16 + mi;
  if (i < Cin) {
    float *row = grad_W + ((int64_t)l * Cin + i) * Cout;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int o = o0 + t * 16 + 4 * mh;
      if (o < Cout) *reinterpret_cast<f32x4 *>(row + o) = acc[t];
    }
  }
}

bool size_ok(int64_t c) { return c >= 16 && c <= 512 && c % 16 == 0; }

template <int NS, int NCT, int GK, bool TW>
int launch_conv(const float *coef, const float *W, float *out, int batch, int lmax, int K, int N, hipStream_t st) {
  const size_t lds = (size_t)NS * NCT * 16 * (round32(K) + kPad) * sizeof(__bf16);
  if (lds > 64 * 1024)
    GWEN_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_spectral_conv<NS, NCT, GK, TW>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // tiles a block: as many as leave about four blocks a CU (every block stages its W panel again), 16 at most
  const int64_t ctiles = (N + NCT * 16 - 1) / (NCT * 16);
  const int64_t rows = (int64_t)batch * (lmax + 1) * (lmax + 1);
  const int64_t all = (rows / kRows + (lmax + 1) / 2 + 1) * ctiles;      // ~ sum over degrees of ceil(rows_l / 64)
  int tpb = (int)(all / 1024);
  tpb = tpb < 1 ? 1 : (tpb > kMaxTilesPerBlock ? kMaxTilesPerBlock : tpb);
  const int64_t tiles = ((int64_t)batch * (2 * lmax + 1) + kRows - 1) / kRows;     // of the last degree, the longest
  const dim3 grid((unsigned)((tiles + tpb - 1) / tpb), (unsigned)(lmax + 1), (unsigned)ctiles);
  k_spectral_conv<NS, NCT, GK, TW><<<grid, kThreads, lds, st>>>(coef, W, out, batch, lmax, K, N, tpb);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}

// the load group grows with K: 2 k-steps up to 64, 4 up to 128, 8 beyond (64 registers a group, two groups live)
template <int NS, bool TW>
int launch_conv_ns(const float *coef, const float *W, float *out, int batch, int lmax, int K, int N, hipStream_t st) {
  if (K <= 64) return launch_conv<NS, 4, 2, TW>(coef, W, out, batch, lmax, K, N, st);
  if (K <= 128) return launch_conv<NS, 4, 4, TW>(coef, W, out, batch, lmax, K, N, st);
  if (K <= 256) return launch_conv<NS, 4, 8, TW>(coef, W, out, batch, lmax, K, N, st);
  return launch_conv<NS, 2, 8, TW>(coef, W, out, batch, lmax, K, N, st);
}

// sizes every entry point shares; GWEN_OK, or the error to return
int check_sizes(int64_t batch, int64_t lmax, int64_t Cin, int64_t Cout, int contract) {
  if (batch < 0 || lmax < 0 || lmax > 1023) return GWEN_EINVAL;
  if (!gwen_spectral_conv_supported(Cin, Cout, contract)) return GWEN_EINVAL;
  if (batch > INT32_MAX / (2 * lmax + 1)) return GWEN_ERANGE;        // a degree's row count fits int32
  return GWEN_OK;
}

}  // namespace

extern "C" int gwen_spectral_conv_supported(int64_t Cin, int64_t Cout, int contract) {
  if (contract < 0 || contract > GWEN_CONTRACT_F16X3) return 0;
  const int c = gwen_dense_contract(contract);
  return size_ok(Cin) && size_ok(Cout) && (c == GWEN_CONTRACT_BF16X6 || c == GWEN_CONTRACT_BF16X3) ? 1 : 0;
}

extern "C" int gwen_spectral_conv_f32(const float *coef, const float *W, float *out, int64_t batch, int64_t lmax,
                                      int64_t Cin, int64_t Cout, int transpose_w, int contract, gwen_stream_t stream_) {
  if (transpose_w != 0 && transpose_w != 1) return GWEN_EINVAL;
  const int rc = check_sizes(batch, lmax, Cin, Cout, contract);
  if (rc != GWEN_OK) return rc;
  if (batch == 0) return GWEN_OK;
  if (!coef || !W || !out || coef == out || !gwen_aligned(coef, 16) || !gwen_aligned(W, 16) || !gwen_aligned(out, 16))
    return GWEN_EINVAL;
  hipStream_t st = gwen_stream(stream_);
  const int b = (int)batch, L = (int)lmax, K = (int)Cin, N = (int)Cout;
  if (gwen_dense_contract(contract) == GWEN_CONTRACT_BF16X6)
    return transpose_w ? launch_conv_ns<3, true>(coef, W, out, b, L, K, N, st)
                       : launch_conv_ns<3, false>(coef, W, out, b, L, K, N, st);
  return transpose_w ? launch_conv_ns<2, true>(coef, W, out, b, L, K, N, st)
                     : launch_conv_ns<2, false>(coef, W, out, b, L, K, N, st);
}

extern "C" int gwen_spectral_conv_grad_weight_f32(const float *coef, const float *g, float *grad_W, int64_t batch,
                                                  int64_t lmax, int64_t Cin, int64_t Cout, int contract,
                                                  gwen_stream_t stream_) {
  const int rc = check_sizes(batch, lmax, Cin, Cout, contract);
  if (rc != GWEN_OK) return rc;
  if (batch == 0) return GWEN_OK;                                     // nothing is launched: grad_W is left as it is
  if (!grad_W || !coef || !g || !gwen_aligned(grad_W, 16) || !gwen_aligned(coef, 16) || !gwen_aligned(g, 16))
    return GWEN_EINVAL;
  hipStream_t st = gwen_stream(stream_);
  const dim3 grid((unsigned)(lmax + 1), (unsigned)((Cin + 63) / 64), (unsigned)((Cout + 63) / 64));
  if (gwen_dense_contract(contract) == GWEN_CONTRACT_BF16X6)
    k_spectral_grad_w<3><<<grid, kThreads, 0, st>>>(coef, g, grad_W, (int)batch, (int)lmax, (int)Cin, (int)Cout);
  else
    k_spectral_grad_w<2><<<grid, kThreads, 0, st>>>(coef, g, grad_W, (int)batch, (int)lmax, (int)Cin, (int)Cout);
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}
