// Constants and size rules shared by the U-Net kernels: conv.hip (forward) and conv_bwd.hip (backward).
#pragma once
#include "common.h"
#include "split.h"

namespace {

using gwen::bf16x4;
using gwen::bf16x8;

// an 8 x 16 pixel tile, its 10 x 18 halo patch, 32-channel chunks; LDS images are [pixel][32 channels] with a pixel
// pitch of 48 bf16 = 96 B
constexpr int TH = 8, TW = 16, PH = TH + 2, PW = TW + 2, kPatch = PH * PW, CK = 32, PITCH = 48, kThreads = 256;
constexpr int kFrag = 64 * 8;                 // bf16 elements of one packed fragment (64 lanes x 8)
constexpr int64_t kMaxC = 2048;

inline bool split_contract(int contract) {
  return contract == GWEN_CONTRACT_BF16X3 || contract == GWEN_CONTRACT_BF16X6 || contract == GWEN_CONTRACT_F16X3;
}
constexpr int64_t k4GiB = int64_t(1) << 32;
// rows x ld fp32 elements addressable below 4 GiB (larger tensors: GWEN_ERANGE, a follow-up)
inline bool fits(int64_t rows, int64_t ld) { return rows == 0 || ld <= k4GiB / 4 / rows; }

// the two-stage per-channel fp64 sums (gwen_channel_stats_f64, gwen_norm_relu_backward_f32): rows per stage-1 chunk
constexpr int kStatLanes = 4;
inline int64_t stat_chunk_rows(int64_t rows) {
  int64_t r = (rows + 511) / 512;
  r = (r + kStatLanes - 1) / kStatLanes * kStatLanes;
  return r < 32 ? 32 : r;
}
inline int64_t stat_chunks(int64_t rows) { const int64_t r = stat_chunk_rows(rows); return (rows + r - 1) / r; }

}  // namespace
