// Packed W for the narrow K4 / K5 forward kernels: the bf16 images of a weight, cut once per weight version instead of
// once per wave of every block of every launch (layer.hip, chain.hip: PK).
//
// A wave of K4 / K5 holds the B fragments of ITS 16 output columns: lane (mi, mh) = (lane & 15, lane >> 4) holds
// W[16 j + mi][KF (4 ks + mh) .. +KF) of column tile j and k-step ks, as NS bf16 images (split.h).  The packed form stores
// exactly these registers, in the order a wave reads them:
//     [column tile j][k-step ks][image s][lane][KF]        bf16, Fout * Fin * NS elements
// so one (j, ks, s) fragment is one contiguous run (1 KiB at KF = 8) that a wave loads with a single 16-byte-per-lane
// instruction (8 bytes at KF = 4, Fin = 16).  The images are cut by the same gwen::split_images the kernels call: a
// kernel that reads them computes bit for bit what it computes from W itself.
#include "common.h"
#include "split.h"

namespace {

template <int K> using BF = gwen::BFv<K>;

// one thread per (j, ks, lane): the thread writes what that lane of the forward kernels holds
template <int KF, int NS>
__global__ __launch_bounds__(64) void k_pack_w(const float *__restrict__ W, __bf16 *__restrict__ P, int32_t fin,
                                              int32_t fout) {
  const int ks_n = fin / (4 * KF);
  const int lane = threadIdx.x, mi = lane & 15, mh = lane >> 4;
  const int ks = blockIdx.x % ks_n, j = blockIdx.x / ks_n;
  if (j * 16 + mi >= fout) return;                          // never: the grid is Fout / 16 column tiles of whole k-steps
  const float *wp = W + (int64_t)(j * 16 + mi) * fin + KF * (4 * ks + mh);
  float wv[KF];
#pragma unroll
  for (int i = 0; i < KF; ++i) wv[i] = wp[i];
  typename BF<KF>::T im[NS];
  gwen::split_images<KF, NS>(wv, im);
#pragma unroll
  for (int s = 0; s < NS; ++s)
    *reinterpret_cast<typename BF<KF>::T *>(P + ((int64_t)((j * ks_n + ks) * NS + s) * 64 + lane) * KF) = im[s];
}

constexpr bool width_ok(int64_t f) { return f == 16 || f == 32 || f == 64; }

}  // namespace

extern "C" int64_t gwen_gcn_packw_bytes(int64_t Fin, int64_t Fout, int contract) {
  if (!width_ok(Fin) || !width_ok(Fout)) return 0;
  if (contract != GWEN_CONTRACT_BF16X3 && contract != GWEN_CONTRACT_BF16X6) return 0;
  return Fin * Fout * gwen::images_of(contract) * 2;
}

extern "C" int gwen_gcn_packw_f32(const float *W, int64_t Fin, int64_t Fout, int contract, void *packed,
                                  gwen_stream_t stream) {
  if (gwen_gcn_packw_bytes(Fin, Fout, contract) == 0) return GWEN_EINVAL;
  if (!W || !packed || !gwen_aligned(W, 16) || !gwen_aligned(packed, 16)) return GWEN_EINVAL;
  const int kf = Fin >= 32 ? 8 : 4;
  const unsigned blocks = (unsigned)((Fout / 16) * (Fin / (4 * kf)));
  __bf16 *P = static_cast<__bf16 *>(packed);
  hipStream_t st = gwen_stream(stream);
  const int32_t fi = (int32_t)Fin, fo = (int32_t)Fout;
  if (contract == GWEN_CONTRACT_BF16X6) {
    if (kf == 8) k_pack_w<8, 3><<<blocks, 64, 0, st>>>(W, P, fi, fo);
    else k_pack_w<4, 3><<<blocks, 64, 0, st>>>(W, P, fi, fo);
  } else {
    if (kf == 8) k_pack_w<8, 2><<<blocks, 64, 0, st>>>(W, P, fi, fo);
    else k_pack_w<4, 2><<<blocks, 64, 0, st>>>(W, P, fi, fo);
  }
  GWEN_LAUNCH_CHECK();
  return GWEN_OK;
}
