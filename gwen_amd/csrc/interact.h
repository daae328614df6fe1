// K6's host interface between its two translation units: interact.hip validates a call (gwen_mlp2_ln_f32,
// gwen_mlp2_bwd_contract_f32) and launches k_mlp2 at 32 and 128 channels; interact_rows.hip launches the row-stationary
// k_mlp2r at 64 and 256 channels, forward and edge backward.  What both must agree on lives here and nowhere else.
#pragma once
#include "common.h"
#include "dispatch.h"

// how table G1 / G2 is addressed (kernel template arguments M1 / M2): absent, row r itself, row idx[r]
constexpr int kNone = 0, kSelf = 1, kIdx = 2;
// the pairs (M1, M2) that are built, as one dispatch list of 3 M1 + M2 (gwen_hip.h lists them for the caller)
using Mlp2Pairs = gwen::ints<3 * kNone + kNone, 3 * kSelf + kNone, 3 * kIdx + kNone, 3 * kIdx + kIdx>;
// the residual of k_mlp2r (template argument RES): none, the A rows themselves, other rows
constexpr int kResNone = 0, kResA = 1, kResOther = 2;
// most rows a pass of either kernel takes: what the 32-bit row arithmetic leaves free below 2^31, and the largest tile
// gwen_edge_tiles cuts.  Each file asserts it against its own MCfg / RCfg.
constexpr int kMaxRows = 128;

struct Mlp2Mode {              // which instantiation: width, table addressing, f16x3 instead of 3xbf16
  int F, m1, m2, f16;
};

struct Mlp2Args {              // a validated forward launch, as gwen_mlp2_ln_f32 names it
  const float *A, *W1, *G1;
  const int32_t *idx1;
  const float *G2;
  const int32_t *idx2;
  const float *b1, *W2, *b2, *res;
  float *out;
  int64_t R;
  int act;
  const int32_t *rowptr, *tile_row;
  int64_t n_tiles;
  float *agg;
  int mean;
  void *workspace;
  uint32_t ldb1, ldb2;         // row pitches of G1 / G2 in bytes
  const float *ln_g, *ln_b;    // both or neither
  float ln_eps;
  hipStream_t st;
};

struct Mlp2BwdArgs {           // a validated edge backward, as gwen_mlp2_bwd_contract_f32 names it (hid = g_pre1, out = g_e)
  const float *ge, *W2t, *d1, *T;
  const int32_t *dst;
  const float *Wet;
  float *hid, *out;
  int64_t R;
  void *workspace;
  uint32_t ldbT;               // row pitch of T in bytes
  hipStream_t st;
};

// interact_rows.hip
int gwen_mlp2_rows_f();                                     // rows a pass of k_mlp2r takes
int64_t gwen_mlp2_rows_ws_bytes(int F, int f16);            // its workspace (256 channels only)
int gwen_mlp2_rows_launch(const Mlp2Mode &m, const Mlp2Args &a);             // m.F in {64, 256}
int gwen_mlp2_rows_bwd_launch(int F, int f16, const Mlp2BwdArgs &a);         // F in {64, 256}
