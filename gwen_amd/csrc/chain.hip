// K5 -- K4 with the NEXT layer's projection chained on, and the "activation first" variant.
//
// A~ is linear, so each GCNConv layer may run transform-first (PyG's order: h = x W^T, then
// aggregate at width Fout) or aggregate-first (aggregate at width Fin, then project); the gather --
// the HBM/fabric-bound part -- is cheapest at min(Fin, Fout).  To gather a SHRINKING layer
// (Fout < Fin) at Fout, its projection has to exist before its gather starts: this kernel appends it
// to the kernel that produces the layer's input, while the rows are still in LDS:
//
//   PRE = 0:  t1 = act(A~ x W1^T + b) ;  out = t1 W2^T          (layer l, then layer l+1's `lin`)
//   PRE = 1:  t0 = act(A~ h + b)      ;  out = t0 W1^T          (layer l was pre-projected: bias and
//                                                                 ReLU come BEFORE the contraction,
//                                                                 which is layer l+1's `lin`)
// e.g. GNNModel(C=64,H=64) = 64->64->32->16->32->64->64 runs as
//   [gather 64, W1, b1+ReLU, W2 -> 32] [gather 32, b2+ReLU, W3 -> 16] [gather 16, b3+ReLU]
//   [gather 16, W4, ...] [gather 32, W5, ...] [gather 64, W6, ...]   -- gathered widths 64,32,16,16,32,64
// instead of 64,64,32,16,32,64 (reference call sites: /root/reference/src/gwen/models_gnn.py:147-149,
// :204-206; the re-bracketing only changes fp32 rounding order).
// Structure, layout, contraction (bf16 split with NS images per operand, fp32 accumulate: split.h) and numerics
// are K4's (layer.hip), and so is the prologue: raw W1 / W2 loads and an unconditional bias load first, nothing waits
// for them, the first index request right behind; the split into images goes to gather_passes' shadow callable
// (chain_pin says per shape whether it is pinned under the first row loads or left to the optimiser from there on).
// k_gather loads its bias above the gather as well (from x when there is none; nothing is added then), not in the sink,
// where it was a dependent round trip at the tail of every wave.
// Stores (template argument ST of k_chain and k_gather; gather_rows.h, store_out): as K4's -- 1 plain, 3 the same 16-byte
// stores written through (sc1), at both store sites of k_chain (phase 2 when nothing is chained, phase 3) and in k_gather's
// sink.  Which shapes run 3: chain_store_mode.  Modes 2 / 4 (whole rows through LDS) are not built.
#include "common.h"
#include "dispatch.h"
#include "gather_rows.h"
#include "split.h"

namespace {

constexpr int kTile = 16;
using gwen::bf16x4;
using gwen::bf16x8;
template <int K> using BF = gwen::BFv<K>;

constexpr int pitch_bf16(int f) { return ((f / 2) % 16 == 8 ? f / 2 : f / 2 + 8) * 2; }

// B fragments (NS images) of output-column tile j of a [FO, FI] weight: W[16 j + mi][KF (4 ks + mh) .. +KF)
// PK: the images come from the weight's packed form (packw.hip) -- load_packed, then pin in the shadow; no raw, no split
template <int FI, int NS, bool PK = false>
struct Frag {
  static constexpr int KF = FI >= 32 ? 8 : 4;
  static constexpr int KS = FI / (4 * KF);
  using T = typename BF<KF>::T;
  T im[KS][NS];
  struct NoRaw {};
  std::conditional_t<PK, NoRaw, float4_t[KS][KF / 4]> raw;   // load_raw .. split: W as loaded (dead afterwards); packed: none
  // packed: the images themselves, [j][ks][s][lane][KF] -- one contiguous run per fragment (issued at the top of the kernel)
  __device__ __forceinline__ void load_packed(const float *W, int j, int lane) {
    const __bf16 *wp = reinterpret_cast<const __bf16 *>(W) + ((int64_t)j * KS * NS * 64 + lane) * KF;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int s = 0; s < NS; ++s) im[ks][s] = *reinterpret_cast<const T *>(wp + (ks * NS + s) * 64 * KF);
  }
  // load in two halves: the loads alone (issued at the top of the kernel), and the split into images (in the shadow
  // of the first row loads, gather_rows.h); together they are load()
  __device__ __forceinline__ void load_raw(const float *W, int j, int mi, int mh) {
    const float *wrow = W + (int64_t)(j * 16 + mi) * FI;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int i = 0; i < KF; i += 4)
        raw[ks][i / 4] = *reinterpret_cast<const float4_t *>(wrow + KF * (4 * ks + mh) + i);
  }
  __device__ __forceinline__ void split() {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      float wv[KF];
#pragma unroll
      for (int i = 0; i < KF; i += 4)
#pragma unroll
        for (int e = 0; e < 4; ++e) wv[i + e] = raw[ks][i / 4][e];
      gwen::split_images<KF, NS>(wv, im[ks]);
    }
  }
  __device__ __forceinline__ void pin() {                  // after split(): the split stays where it was written
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int s = 0; s < NS; ++s) gwen::pin_here(im[ks][s]);
  }
  // d += W-fragment (A operand) x tile rows arow.. from the NS LDS images, `img` elements apart (B operand): the
  // product comes out TRANSPOSED -- lane (mi, mh) holds row mi, columns 16 j + 4 mh .. +3
  __device__ inline f32x4 mma(const __bf16 *t, int img, int arow, int mh, f32x4 d) const {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      T a[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) a[s] = *reinterpret_cast<const T *>(t + s * img + arow + KF * (4 * ks + mh));
      d = gwen::mma_split<KF, NS>(im[ks], a, d);
    }
    return d;
  }
};

// The block geometry of K5 -- the one copy of the rule.  Plain ints in, so the kernels read it at compile time (Cfg) and
// the extern "C" checks at run time (rows_valid, gwen_gcn_chain_supported).  brq: Cfg's BRQ.
struct Geom {
  int G, R;                                                // lanes per gathered row, rows per wave pass
  int NWB, RB;                                             // waves per block, rows gathered per block pass
  int BRMIN, BR;                                           // rows per block: asked for, and had (whole gather passes)
  int PB0, PB1;                                            // row pitch (bf16) of the aggregated rows', the first product's images
  // bf16x6 (three images): the first product's images take the place of the aggregated rows' (one more barrier,
  // the product waits in registers meanwhile) -- with both sets resident 64 -> 64 -> 32 kept two blocks per CU
  // instead of three and ran 30.5 us against 22.9 for bf16x3
  bool ALIAS;
  size_t img0, img1, lds_elems;                            // bf16 elements: either set of images, one block
  constexpr Geom(int fin, int f1, int f2, int ns, int brq)
      : G(fin / 4), R(64 / (fin / 4)), NWB(f1 / 16 > 4 ? 8 : 4), RB(NWB * R), BRMIN(fin >= 128 ? 128 : brq),
        BR(RB > BRMIN ? RB : BRMIN), PB0(pitch_bf16(fin)), PB1(pitch_bf16(f1)), ALIAS(ns == 3 && f2 > 0),
        img0((size_t)ns * BR * PB0), img1(f2 > 0 ? (size_t)ns * BR * PB1 : 0),
        lds_elems(ALIAS ? (img0 > img1 ? img0 : img1) : img0 + img1) {}
  constexpr bool fits(size_t lds_bytes) const { return lds_elems * 2 <= lds_bytes; }
};
constexpr size_t kLdsCU = 160 * 1024;                      // LDS of a CU

// FIN: gathered width.  F1: width after the first contraction.  F2: width after the second (0: none).
// BRQ: rows per block asked for below 128 channels (64; 96 / 112 where they are whole gather passes: rows_ok)
template <int FIN, int F1, int F2, bool PRE, int NS, int BRQ = 64>
struct Cfg {
  static constexpr Geom geo = Geom(FIN, F1, F2, NS, BRQ);
  static constexpr int G = geo.G, R = geo.R;
  static constexpr int NJ1 = F1 / 16, NJ2 = F2 / 16;
  static constexpr int NWB = geo.NWB, RB = geo.RB, BRMIN = geo.BRMIN, BR = geo.BR;
  static constexpr int NP = BR / RB, NT = BR / kTile;
  static_assert(BR % RB == 0 && BR % kTile == 0, "a block is whole gather passes and whole row tiles");
  static constexpr int PB0 = geo.PB0, PB1 = geo.PB1;
  static constexpr int FW = F2 > 0 ? F2 : F1;              // stored width
  static constexpr bool ALIAS = geo.ALIAS;
  static constexpr size_t img0 = geo.img0, img1 = geo.img1, lds_elems = geo.lds_elems;
  static_assert(!(PRE && F2 > 0), "activation-first has one contraction");
  static_assert(NWB % NJ1 == 0 && (F2 == 0 || NWB % NJ2 == 0), "waves must tile the columns");
};

// The W slices are split into bf16 images in gather_passes' shadow callable (gather_rows.h).  true: the images are pinned
// there (split.h, pin_here), under the first row loads; false: the optimiser may sink the split from there to the images'
// first use, the tail of the gather -- fewer registers.  Per (Fin, F1, F2, images), from the registers (no c2 kernel may
// lose a wave of occupancy) and the per-kernel measurement on the MI355X (profiles/prologue_*, DESIGN 4 K4 "Prologue"):
// 64 -> 64 -> 32 on bf16x6 is pinned (160 VGPRs, still 3 waves); pinned, 32 -> 16 holds 81 VGPRs and loses its 6th wave.
// Only with 7 gathered entries, the measured form: with 8 the pinned images take the kernel from 3 waves to 2.
constexpr bool chain_pin(int fin, int f1, int f2, int ns, int ge) {
  return fin == 64 && f1 == 64 && f2 == 32 && ns == 3 && ge == 7;
}

// GE: gathered entries per group (gather_rows.h; 7 only on the uniform layout).  D: gather depth (gather_rows.h).
// BRQ: Cfg's.  IM: index mode (gather_rows.h; 2 = index records: narrow kernels on the uniform layout only).  They sit
// before NS because profile tooling keys this kernel's name on its first and its last template argument.
// PK: packed W (packw.hip; narrow kernels only): W1 and W2 point to the weights' bf16 images in fragment order and the B
// fragments are plain loads at the top of the kernel.  false compiles to the code the kernel had.
// ST: store mode of both store sites -- phase 2 at F2 == 0, and phase 3 (gather_rows.h, store_out): 1 = plain 16-byte
// stores, the code the kernel had; 3 = the same addresses written through.  Narrow kernels on the uniform layout only;
// in front of NS for the reason above.
template <int FIN, int F1, int F2, bool PRE, bool UNI, int GE, int D, int BRQ, int IM, bool PK, int ST, int NS>
__global__ __launch_bounds__((F1 > 64 ? 512 : 256)) void k_chain(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const float *__restrict__ val, const float *__restrict__ x, const float *__restrict__ W1,
    const float *__restrict__ W2, const float *__restrict__ bias, float *__restrict__ out, int32_t N,
    int64_t mstride_x, int64_t mstride_o, int relu) {
  using C = Cfg<FIN, F1, F2, PRE, NS, BRQ>;
  static_assert(IM == 1 || (IM == 2 && UNI && FIN <= 64 && F1 <= 64), "index records: narrow kernels, uniform layout");
  static_assert(!PK || (FIN <= 64 && F1 <= 64), "packed W: narrow kernels");
  static_assert(ST == 1 || (ST == 3 && UNI && FIN <= 64 && F1 <= 64), "store modes: narrow kernels, uniform layout");
  __shared__ __attribute__((aligned(16))) __bf16 lds[C::lds_elems];
  constexpr int kImg0 = C::BR * C::PB0, kImg1 = C::BR * C::PB1;
  __bf16 *t0 = lds;                                                      // aggregated rows: NS x [BR][PB0]
  __bf16 *t1 = C::ALIAS ? lds : lds + NS * kImg0;                        // first product:   NS x [BR][PB1]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int gl = lane % C::G, gr = lane / C::G;
  const int mi = lane & 15, mh = lane >> 4;

  const int nb = gridDim.x, bid = blockIdx.x;
  const int xcd = bid & 7, q8 = nb >> 3, r8 = nb & 7;
  const int lb = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const int b0 = lb * C::BR;

  const char *xb = reinterpret_cast<const char *>(x + (int64_t)blockIdx.y * mstride_x);
  float *om = out + (int64_t)blockIdx.y * mstride_o;
  const uint32_t lane_off = gl * 16;

  // weights of both contractions for this wave's column tiles: the raw loads are issued here, before the first index
  // request and with no wait behind them; they are split into images in the shadow of the first row
  // loads (gather_rows.h; chain_pin says whether pinned there).  Bias: never a load under a condition (gather_rows.h) --
  // without one the same 16 bytes of W1 are read (F1 * FIN floats: at least FIN, at least F1) and masked to +0.
  constexpr bool kPin = chain_pin(FIN, F1, F2, NS, GE);
  const int j1 = wave % C::NJ1;
  Frag<FIN, NS, PK> b1;
  if constexpr (PK) b1.load_packed(W1, j1, lane);
  else b1.load_raw(W1, j1, mi, mh);
  const int j2 = wave % (F2 > 0 ? C::NJ2 : 1);
  Frag<(F2 > 0 ? F1 : 16), NS, PK> b2;
  if constexpr (F2 > 0) {
    if constexpr (PK) b2.load_packed(W2, j2, lane);
    else b2.load_raw(W2, j2, mi, mh);
  }
  float4_t bpre = {0.f, 0.f, 0.f, 0.f}, bpost = {0.f, 0.f, 0.f, 0.f};
  float4_t braw = *reinterpret_cast<const float4_t *>((bias ? bias : W1) + (PRE ? gl * 4 : j1 * 16 + 4 * mh));
  // the mask waits for the load, so it is applied in the shadow callable, not here
  auto split_w = [&]() {
    (PRE ? bpre : bpost) = gwen::masked_f4(braw, bias != nullptr);
    gwen::pin_here(PRE ? bpre : bpost);                    // or mask and load sink to the value's first use
    if constexpr (!PK) {
      b1.split();
      if constexpr (F2 > 0) b2.split();
    }
    if constexpr (kPin || PK) {                            // packed: the image loads stay at the top, their values are due here
      b1.pin();
      if constexpr (F2 > 0) b2.pin();
    }
  };
  __builtin_amdgcn_sched_barrier(0);                       // the raw loads stay in front of the first index request

  // ---- phase 1: gather + aggregate (+ bias, ReLU when activation-first) -> LDS hi/lo -------------
  auto sink = [&](int lr, float4_t acc) {
        if constexpr (PRE) {
          acc = acc + bpre;
          if (relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = acc[e] < 0.0f ? 0.0f : acc[e];
          }
        }
        const float a4[4] = {acc[0], acc[1], acc[2], acc[3]};
        bf16x4 im[NS];
        gwen::split_images<4, NS>(a4, im);
#pragma unroll
        for (int s = 0; s < NS; ++s) *reinterpret_cast<bf16x4 *>(t0 + s * kImg0 + lr * C::PB0 + gl * 4) = im[s];
      };
  gwen::gather_passes<FIN, C::NP, C::RB, UNI, GE, D, IM>(rowptr, col, val, xb, N, b0, wave, gr, lane_off, sink, split_w);
  __syncthreads();

  // ---- phase 2: first contraction; result to global (F2 == 0) or to the second LDS image ----------
  constexpr int TS1 = C::NWB / C::NJ1;                                   // row tiles are strided over the waves
  constexpr int NIT = (C::NT + TS1 - 1) / TS1;                           // row tiles of this wave (at most)
  float4_t keep[C::ALIAS ? NIT : 1];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int tt = wave / C::NJ1 + it * TS1;
    if (C::NT % TS1 != 0 && tt >= C::NT) continue;                       // 96 / 112 rows: the last stride is partial
    f32x4 d = {0.f, 0.f, 0.f, 0.f};
    d = b1.mma(t0, kImg0, (tt * kTile + mi) * C::PB0, mh, d);
    const int lr = tt * kTile + mi;
    float4_t o = {d[0], d[1], d[2], d[3]};
    if constexpr (!PRE) {
      o = o + bpost;
      if (relu) {
#pragma unroll
        for (int t = 0; t < 4; ++t) o[t] = o[t] < 0.0f ? 0.0f : o[t];
      }
    }
    if constexpr (C::ALIAS) {
      keep[it] = o;
    } else if constexpr (F2 > 0) {
      const float o4[4] = {o[0], o[1], o[2], o[3]};
      bf16x4 im[NS];
      gwen::split_images<4, NS>(o4, im);
#pragma unroll
      for (int s = 0; s < NS; ++s)
        *reinterpret_cast<bf16x4 *>(t1 + s * kImg1 + lr * C::PB1 + j1 * 16 + 4 * mh) = im[s];
    } else {
      if (b0 + lr < N) gwen::store_out<ST>(om + (int64_t)(b0 + lr) * F1 + j1 * 16 + 4 * mh, o);
    }
  }
  if constexpr (C::ALIAS) {
    __syncthreads();                                   // every wave is done reading the aggregated rows
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      if (C::NT % TS1 != 0 && wave / C::NJ1 + it * TS1 >= C::NT) continue;
      const int lr = (wave / C::NJ1 + it * TS1) * kTile + mi;
      const float o4[4] = {keep[it][0], keep[it][1], keep[it][2], keep[it][3]};
      bf16x4 im[NS];
      gwen::split_images<4, NS>(o4, im);
#pragma unroll
      for (int s = 0; s < NS; ++s)
        *reinterpret_cast<bf16x4 *>(t1 + s * kImg1 + lr * C::PB1 + j1 * 16 + 4 * mh) = im[s];
    }
  }
  if constexpr (F2 > 0) {
    __syncthreads();
    // ---- phase 3: second contraction (the next layer's `lin`), stored at width F2 ---------------
#pragma unroll
    for (int tt = wave / C::NJ2; tt < C::NT; tt += C::NWB / C::NJ2) {
      f32x4 d = {0.f, 0.f, 0.f, 0.f};
      d = b2.mma(t1, kImg1, (tt * kTile + mi) * C::PB1, mh, d);
      const int r = b0 + tt * kTile + mi;
      if (r < N) gwen::store_out<ST>(om + (int64_t)r * F2 + j2 * 16 + 4 * mh, float4_t{d[0], d[1], d[2], d[3]});
    }
  }
}

// Activation-first layer with nothing chained: out = act(A~ h + bias) on the grouped layout (the
// fma form of K2; K2 itself keeps the rounded-product order that is bit-identical to the CPU path).
// D: accepted for symmetry with K4 / K5 -- a wave gathers ONE pass here, so both depths are the same code
// ST: store mode (gather_rows.h, store_out): the rows are stored whole already, so 1 (plain) and 3 (written through) only
template <int FIN, bool UNI, int GE = 8, int D = 1, int IM = 1, int ST = 1>
__global__ __launch_bounds__(256) void k_gather(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const float *__restrict__ val, const float *__restrict__ x, const float *__restrict__ bias,
    float *__restrict__ out, int32_t N, int64_t mstride_x, int64_t mstride_o, int relu) {
  constexpr int G = FIN / 4, R = 64 / G, BR = 4 * R;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int gl = lane % G, gr = lane / G;
  const int nb = gridDim.x, bid = blockIdx.x;
  const int xcd = bid & 7, q8 = nb >> 3, r8 = nb & 7;
  const int lb = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const char *xb = reinterpret_cast<const char *>(x + (int64_t)blockIdx.y * mstride_x);
  float *om = out + (int64_t)blockIdx.y * mstride_o;
  const uint32_t lane_off = gl * 16;
  // bias: loaded above the gather (the oldest load: no later wait is longer for it) and never under a condition
  // (gather_rows.h) -- without one the first row of x is read (N >= 1: at least FIN floats) and nothing is added:
  // acc + 0 would turn an aggregated -0 into +0
  const float4_t braw = *reinterpret_cast<const float4_t *>(bias ? reinterpret_cast<const char *>(bias) + lane_off
                                                                 : xb + lane_off);
  __builtin_amdgcn_sched_barrier(0);
  gwen::gather_passes<FIN, 1, BR, UNI, GE, D, IM>(
      rowptr, col, val, xb, N, lb * BR, wave, gr, lane_off, [&](int lr, float4_t acc) {
        if (bias) acc = acc + braw;
        if (relu) {
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = acc[e] < 0.0f ? 0.0f : acc[e];
        }
        if (lb * BR + lr < N) gwen::store_out<ST>(om + (int64_t)(lb * BR + lr) * FIN + gl * 4, acc);
      });
}

// What one K5 launch (k_chain or k_gather) works on; gwen_gcn_chain_tuned_f32 fills it once.
struct ChainArgs {
  const int32_t *rowptr, *col;                             // rowptr NULL = uniform layout
  const float *val, *x, *W1, *W2, *bias;                   // W1, W2: the weights, or their packed images (launch_br<.., PK>)
  float *out;
  int64_t N, members, msx, mso;
  int relu, entries;
  int store_mode;                                          // 1 or 3, resolved (k_chain's / k_gather's ST)
  hipStream_t st;
  int *probe;                                              // not NULL: launch nothing, store the kernel's blocks per CU
};

constexpr bool narrow(int fin, int f1) { return fin <= 64 && f1 <= 64; }
constexpr int gather_rows(int fin) { return 4 * Geom(fin, 0, 0, 2, 64).R; }   // k_gather's block: one pass of four waves

// rows per block that the narrow kernels (Fin, F1 <= 64) can be asked for: whole gather passes; at 112 rows the largest
// of them, 64 -> 64 -> 32 on bf16x3, holds 70 KiB of LDS.  Decides which launch_br are instantiated and, with the kernel's
// own size, what block_rows a caller may force.
// pk: the packed-W kernels also have 80 rows (Fin = 64: five passes), as K4's -- only through the entry points that take
// images; every older entry point keeps refusing 80
constexpr bool rows_ok(int fin, int f1, int br, bool pk = false) {
  return narrow(fin, f1) && (br == 64 || (br == 80 && pk) || br == 96 || br == 112) && br % Geom(fin, f1, 0, 2, 64).RB == 0;
}

// block_rows of gwen_gcn_chain_tuned_f32: 0, the kernel's own size, or 96 / 112 on the narrow kernels.  plain: k_gather
constexpr bool rows_valid(int fin, int f1, bool plain, int br, bool pk = false) {
  if (br == 0) return true;
  if (plain) return br == gather_rows(fin);
  return br == Geom(fin, f1, 0, 2, 64).BR || rows_ok(fin, f1, br, pk);
}

// gathered entries: 7 only on the uniform layout, when the caller promises it, on widths up to 64
template <int FIN, int D, int IM>
int launch_gather(const ChainArgs &a) {
  constexpr int BR = gather_rows(FIN);
  dim3 grid((unsigned)((a.N + BR - 1) / BR), (unsigned)a.members);
  auto run = [&](auto kernel) {
    kernel<<<grid, 256, 0, a.st>>>(a.rowptr, a.col, a.val, a.x, a.bias, a.out, (int32_t)a.N, a.msx, a.mso, a.relu);
    GWEN_LAUNCH_CHECK();
    return (int)GWEN_OK;
  };
  if constexpr (FIN <= 64 && D == 1) {         // written through: the uniform layout, up to 64 channels (both depths are one code)
    if (a.store_mode == 3) {
      if (a.rowptr) return GWEN_EINVAL;
      return a.entries == 7 ? run(&k_gather<FIN, true, 7, 1, IM, 3>) : run(&k_gather<FIN, true, 8, 1, IM, 3>);
    }
  }
  if (a.store_mode != 1) return GWEN_EINVAL;
  if constexpr (IM == 2) {                     // index records: the uniform layout, up to 64 channels
    if (a.rowptr) return GWEN_EINVAL;
    return a.entries == 7 ? run(&k_gather<FIN, true, 7, D, 2>) : run(&k_gather<FIN, true, 8, D, 2>);
  }
  if (a.rowptr) return run(&k_gather<FIN, false, 8, D>);
  if constexpr (FIN <= 64) {
    if (a.entries == 7) return run(&k_gather<FIN, true, 7, D>);
  }
  return run(&k_gather<FIN, true, 8, D>);
}

template <int FIN, int F1, int F2, bool PRE, int NS, int D, int BRQ, int IM, bool PK, int ST>
int launch_br(const ChainArgs &a) {
  using C = Cfg<FIN, F1, F2, PRE, NS, BRQ>;
  static_assert(C::geo.fits(kLdsCU), "one block must fit a CU's LDS");
  dim3 grid((unsigned)((a.N + C::BR - 1) / C::BR), (unsigned)a.members);
  auto run = [&](auto kernel) {
    if (a.probe) {
      GWEN_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(a.probe, reinterpret_cast<const void *>(kernel),
                                                                  C::NWB * 64, 0));
      return (int)GWEN_OK;
    }
    kernel<<<grid, C::NWB * 64, 0, a.st>>>(a.rowptr, a.col, a.val, a.x, a.W1, a.W2, a.bias, a.out, (int32_t)a.N, a.msx,
                                           a.mso, a.relu);
    GWEN_LAUNCH_CHECK();
    return (int)GWEN_OK;
  };
  if constexpr (IM == 2 || ST != 1) {          // index records, store modes: the uniform layout, narrow kernels
    if (a.rowptr) return GWEN_EINVAL;
    return a.entries == 7 ? run(&k_chain<FIN, F1, F2, PRE, true, 7, D, BRQ, IM, PK, ST, NS>)
                          : run(&k_chain<FIN, F1, F2, PRE, true, 8, D, BRQ, IM, PK, ST, NS>);
  }
  if (a.rowptr) return run(&k_chain<FIN, F1, F2, PRE, false, 8, D, BRQ, 1, PK, 1, NS>);
  if constexpr (narrow(FIN, F1)) {
    if (a.entries == 7) return run(&k_chain<FIN, F1, F2, PRE, true, 7, D, BRQ, 1, PK, 1, NS>);
  }
  return run(&k_chain<FIN, F1, F2, PRE, true, 8, D, BRQ, 1, PK, 1, NS>);
}

// Rows per block of a packed-W kernel (PK) at gather depth 2 where launch_ns would take 112; 0: the same.  64 -> 64 -> 32
// on bf16x6: 80 rows (five passes, 38 400 B of LDS) measured 16.3 us against 17.4 at 112 and at 64 rows
// (profiles/packw_kernel_ab_*); at 156 VGPRs it is three blocks per CU at either size.
constexpr int packed_rows(int fin, int f1, int f2, int ns) { return fin == 64 && f1 == 64 && f2 == 32 && ns == 3 ? 80 : 0; }

// block_rows: 0 = the library's choice; else the kernel's own size or 96 / 112 (rows_ok; checked by the extern "C" caller).
// The library's choice is 64 rows (128 from 128 channels on).  K4's "smallest size whose grid is co-resident" finds no
// such size for the c2 mesh here (64 -> 64 -> 32: 4, 3 and 2 blocks per CU at 64 / 96 / 112 rows against 1 563 / 1 042 /
// 893 blocks) and 96 / 112 rows measured SLOWER at depth 1 (23.3 / 23.5 against 22.2 us), so depth 1 keeps 64.  At depth
// 2 one member whose 64-row grid is more than one resident round runs 112-row blocks where the width allows it: the
// two-deep gather fills and drains once per block (20.1 against 20.8 us).
template <int FIN, int F1, int F2, bool PRE, int NS, int D, int IM, bool PK = false, int ST = 1>
int launch_ns(const ChainArgs &a, int block_rows) {
  static_assert(ST == 1 || narrow(FIN, F1), "store modes: narrow kernels only");
  static_assert(IM == 1 || narrow(FIN, F1), "index records: narrow kernels only");
  static_assert(!PK || narrow(FIN, F1), "packed W: narrow kernels only");
  int brq = block_rows == 0 || block_rows == Cfg<FIN, F1, F2, PRE, NS>::BR ? 64 : block_rows;   // BRQ 64 = the own size
  if constexpr (D == 2 && rows_ok(FIN, F1, 112)) {
    if (block_rows == 0 && a.members == 1) {
      // blocks per CU of the 64-row kernel this call would launch otherwise; probed once per kernel (function-local
      // static): a warm call makes no HIP query, so the launcher stays capturable.  The index mode is part of the
      // kernel (IM = 2 exists on the uniform layout only; launch_br refuses a row pointer)
      static int per_cu[3] = {0, 0, 0};
      const int v = a.rowptr ? 2 : (a.entries == 7 ? 0 : 1);
      if (per_cu[v] == 0) {
        const void *k = v == 2   ? reinterpret_cast<const void *>(&k_chain<FIN, F1, F2, PRE, false, 8, D, 64, 1, PK, 1, NS>)
                        : v == 1 ? reinterpret_cast<const void *>(&k_chain<FIN, F1, F2, PRE, true, 8, D, 64, IM, PK, ST, NS>)
                                 : reinterpret_cast<const void *>(&k_chain<FIN, F1, F2, PRE, true, 7, D, 64, IM, PK, ST, NS>);
        int nbk = 0;
        GWEN_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nbk, k, Cfg<FIN, F1, F2, PRE, NS>::NWB * 64, 0));
        per_cu[v] = nbk < 1 ? 1 : nbk;
      }
      // a packed-W kernel: 80 rows where that measured faster (packed_rows)
      if ((a.N + 63) / 64 > (int64_t)256 * per_cu[v]) brq = PK && packed_rows(FIN, F1, F2, NS) != 0 ? packed_rows(FIN, F1, F2, NS) : 112;
    }
  }
  return gwen::dispatch(gwen::ints<64, 80, 96, 112>{}, brq, [&](auto brv) {
    constexpr int BRQ = decltype(brv)::value;
    if constexpr (BRQ == 64 || rows_ok(FIN, F1, BRQ, PK)) return launch_br<FIN, F1, F2, PRE, NS, D, BRQ, IM, PK, ST>(a);
    else return (int)GWEN_EINVAL;
  });
}

constexpr bool width_ok(int64_t f) { return f == 16 || f == 32 || f == 64 || f == 128; }

}  // namespace

extern "C" int gwen_gcn_chain_supported(int64_t Fin, int64_t F1, int64_t F2, int pre, int contract) {
  if (contract != GWEN_CONTRACT_BF16X3 && contract != GWEN_CONTRACT_BF16X6) return 0;
  const int ns = gwen::images_of(contract);
  if (pre && F1 == 0 && F2 == 0) return width_ok(Fin) ? 1 : 0;      // activation-first, nothing chained
  if (!width_ok(Fin) || !width_ok(F1)) return 0;
  if (pre) return F2 == 0 && Geom(Fin, F1, 0, ns, 64).fits(150 * 1024) ? 1 : 0;   // one block must fit the CU
  if (!(width_ok(F2) && F2 < F1)) return 0;          // chained projection of a SHRINKING next layer
  // worth it only while two blocks still fit a CU's LDS (otherwise K4, then K3 + K2)
  return Geom(Fin, F1, F2, ns, 64).fits(kLdsCU / 2) ? 1 : 0;
}

// The library's gather depth per (Fin, F1, F2, images) on the uniform layout: 2 only where the kernel measured faster
// on the MI355X ("Gather depth"; profiles/depth_*); the non-uniform layout and widths above 64 run depth 1.
static constexpr int chain_depth(int64_t fin, int64_t f1, int64_t f2, int ns) {
  return fin == 64 && f1 == 64 && f2 == 32 && ns == 3 ? 2 : 1;     // 64 -> 64 -> 32 on bf16x6
}

extern "C" int gwen_gcn_chain_depth(int64_t Fin, int64_t F1, int64_t F2, int pre, int contract) {
  if (!gwen_gcn_chain_supported(Fin, F1, F2, pre, contract)) return 0;
  if (!narrow(Fin, F1)) return 1;
  return chain_depth(Fin, F1, F2, gwen::images_of(contract));
}

// The library's index mode per (Fin, F1, F2, pre, images) on the uniform layout (gather_rows.h, IM): 2, one record load
// per row and pass, only where the kernel measured faster on the MI355X ("Index records";
// profiles/index_*); the non-uniform layout and widths above 64 have mode 1 only.
static constexpr int chain_index_mode(int64_t fin, int64_t f1, int64_t f2, int pre, int ns) {
  return fin == 32 && f1 == 16 && f2 == 0 && pre && ns == 3 ? 2 : 1;   // activation-first 32 -> 16 on bf16x6
}

extern "C" int gwen_gcn_chain_index_mode(int64_t Fin, int64_t F1, int64_t F2, int pre, int contract) {
  if (!gwen_gcn_chain_supported(Fin, F1, F2, pre, contract)) return 0;
  if (!narrow(Fin, F1)) return 1;
  return chain_index_mode(Fin, F1, F2, pre, gwen::images_of(contract));
}

// Whether the library's forward reads W1 / W2 as packed images (packw.hip; k_chain's PK) when the caller hands them over,
// per (Fin, F1, F2, pre, images): on only where the kernel measured faster on the MI355X by the rule of the depth and index
// tables ("Packed W"; profiles/packw_*): 64 -> 64 -> 32 (19.7 -> 17.4 us at 112 rows) and activation-first
// 32 -> 16 (8.0 -> 7.0 us), both on bf16x6 -- the two forms of the c2 step.
static constexpr bool chain_packed(int64_t fin, int64_t f1, int64_t f2, int pre, int ns) {
  return ns == 3 && ((fin == 64 && f1 == 64 && f2 == 32 && !pre) || (fin == 32 && f1 == 16 && f2 == 0 && pre));
}

extern "C" int gwen_gcn_chain_packed_mode(int64_t Fin, int64_t F1, int64_t F2, int pre, int contract) {
  if (!gwen_gcn_chain_supported(Fin, F1, F2, pre, contract)) return 0;
  if (!narrow(Fin, F1) || F1 == 0) return 1;              // the form without a contraction reads no W
  return chain_packed(Fin, F1, F2, pre, gwen::images_of(contract)) ? 2 : 1;
}

// The library's store mode per (Fin, F1, F2, pre, images) on the uniform layout (gather_rows.h, store_out): 3, the 16-byte
// output stores written through, only where the kernel measured faster on the MI355X by the rule of the depth and index
// tables ("Stores"; profiles/store_*).  F1 == 0: k_gather.  The modes exist for the narrow kernels on the
// uniform layout at the shape's own depth and index mode; everything else has mode 1 only.
// 64 -> 64 -> 32 and activation-first 32 -> 16 on bf16x6, the only split that was measured, and k_gather<16>, which
// contracts nothing and is one kernel whatever `contract` says (the stack launcher calls it with bf16x3)
// (profiles/store_kernel_ab.tsv).
static constexpr int chain_store_mode(int64_t fin, int64_t f1, int64_t f2, int pre, int ns) {
  if (pre && f1 == 0) return fin == 16 ? 3 : 1;
  return ns == 3 && ((!pre && fin == 64 && f1 == 64 && f2 == 32) || (pre && fin == 32 && f1 == 16 && f2 == 0)) ? 3 : 1;
}

extern "C" int gwen_gcn_chain_store_mode(int64_t Fin, int64_t F1, int64_t F2, int pre, int contract) {
  if (!gwen_gcn_chain_supported(Fin, F1, F2, pre, contract)) return 0;
  if (!narrow(Fin, F1)) return 1;
  return chain_store_mode(Fin, F1, F2, pre, gwen::images_of(contract));
}

// entries = 7: the caller's promise (uniform layout, every row at most 7 stored entries), see gwen_gcn_layer_entries_f32
// depth, block_rows, index_mode: 0 = the library's choice (chain_depth; launch_ns; chain_index_mode); none changes a
// value.  index_mode 1: every lane loads its row's group; 2: index records -- narrow kernels (Fin, F1 <= 64) on the
// uniform layout only, GWEN_EINVAL elsewhere
// W1p, W2p, packed: the gwen_gcn_packw_f32 images of W1 and W2 and whether they are read.  1: the weights are read and
// split in the kernel; 2: the images are read (W1 / W2 may be NULL) -- narrow kernels with a contraction only, and an
// image for every weight the form has, GWEN_EINVAL otherwise; 0: the library's choice -- the images where all of them are
// given and gwen_gcn_chain_packed_mode says 2.  No value changes.
// store_mode: as gwen_gcn_layer_tuned4_f32 -- 0 the library's choice (chain_store_mode, one member only), 1 plain, 3 written
// through (narrow kernels, uniform layout, the shape's own depth and index mode; GWEN_EINVAL elsewhere), 2 and 4 not built
// probe: not NULL = launch nothing and store the blocks per CU that hipOccupancyMaxActiveBlocksPerMultiprocessor reports for
// the kernel this call would launch (forms with a contraction only)
static int chain_tuned(const int32_t *rowptr, const int32_t *col, const float *val,
                       const float *x, const float *W1, const float *W2,
                       const float *bias, float *out, int64_t N, int64_t Fin, int64_t F1,
                       int64_t F2, int pre, int relu, int64_t members, int64_t mstride_x,
                       int64_t mstride_o, int contract, int entries, int depth, int block_rows,
                       int index_mode, const void *W1p, const void *W2p, int packed, int store_mode,
                       gwen_stream_t stream_, int *probe) {
  if (entries != 7 && entries != 8) return GWEN_EINVAL;
  if (store_mode < 0 || store_mode > 4) return GWEN_EINVAL;
  if (packed < 0 || packed > 2) return GWEN_EINVAL;
  if (depth < 0 || depth > 2) return GWEN_EINVAL;
  if (index_mode < 0 || index_mode > 2) return GWEN_EINVAL;
  if (N < 0 || members < 0) return GWEN_EINVAL;
  if (!gwen_gcn_chain_supported(Fin, F1, F2, pre, contract)) return GWEN_EINVAL;
  const bool plain = pre && F1 == 0;                       // activation-first, nothing chained: k_gather
  if (index_mode == 2 && (rowptr || !narrow(Fin, F1))) return GWEN_EINVAL;     // records: uniform layout, narrow kernels
  // store modes: narrow kernels, uniform layout, the shape's own depth (k_gather: either) and index mode; row stores: not built
  const bool can_store = narrow(Fin, F1) && !rowptr &&
                         (plain || depth == 0 || depth == gwen_gcn_chain_depth(Fin, F1, F2, pre, contract)) &&
                         (index_mode == 0 || index_mode == gwen_gcn_chain_index_mode(Fin, F1, F2, pre, contract));
  if (store_mode > 1 && (!can_store || store_mode != 3)) return GWEN_EINVAL;
  if (store_mode == 0) store_mode = can_store && members == 1 ? gwen_gcn_chain_store_mode(Fin, F1, F2, pre, contract) : 1;
  const bool can_pack = !plain && narrow(Fin, F1);                             // packed W: narrow kernels that contract
  const bool have_images = W1p && (F2 == 0 || W2p);
  if (packed == 2 && (!can_pack || !have_images)) return GWEN_EINVAL;
  if (packed == 0) packed = can_pack && have_images && gwen_gcn_chain_packed_mode(Fin, F1, F2, pre, contract) == 2 ? 2 : 1;
  if (packed == 2 && (!gwen_aligned(W1p, 16) || (F2 > 0 && !gwen_aligned(W2p, 16)))) return GWEN_EINVAL;
  if (!rows_valid(Fin, F1, plain, block_rows, packed == 2)) return GWEN_EINVAL;   // the one check of block_rows
  if (packed == 2) {                                       // the images take the weights' places; the checks below hold
    W1 = static_cast<const float *>(W1p);
    W2 = F2 > 0 ? static_cast<const float *>(W2p) : W2;
  }
  if (N == 0 || members == 0) return GWEN_OK;
  if (!col || !val || !x || (F1 > 0 && !W1) || !out || x == out || (F2 > 0 && !W2))
    return GWEN_EINVAL;                                    // rowptr NULL = uniform layout
  if (N >= (int64_t(1) << 28) || members > 65535) return GWEN_ERANGE;
  if (!gwen_aligned(x, 16) || !gwen_aligned(out, 16) || (W1 && !gwen_aligned(W1, 16)) ||
      (W2 && !gwen_aligned(W2, 16)) || (bias && !gwen_aligned(bias, 16)) || mstride_x % 4 || mstride_o % 4)
    return GWEN_EINVAL;                                    // 16-byte loads at x + m * mstride_x, stores at out + m * mstride_o
  if (N * Fin * 4 >= (int64_t(1) << 32)) return GWEN_ERANGE;
  if (depth == 0) depth = rowptr ? 1 : gwen_gcn_chain_depth(Fin, F1, F2, pre, contract);
  if (index_mode == 0) index_mode = rowptr ? 1 : gwen_gcn_chain_index_mode(Fin, F1, F2, pre, contract);
  if (probe && plain) return GWEN_EINVAL;
  const ChainArgs a{rowptr, col, val, x, W1, W2, bias, out, N, members, mstride_x, mstride_o, relu, entries, store_mode,
                    gwen_stream(stream_), probe};
  using Widths = gwen::ints<16, 32, 64, 128>;
  using Depths = gwen::ints<1, 2>;
  using Modes = gwen::ints<1, 2>;
  return gwen::dispatch(Widths{}, Fin, [&](auto fi) {
    constexpr int FI = decltype(fi)::value;
    if (plain) {
      // k_gather is one code at both depths: the written-through form exists once, at depth 1
      return gwen::dispatch(Depths{}, FI <= 64 && store_mode == 1 ? depth : 1, [&](auto dv) {   // gather depth 2: up to 64 channels
        return gwen::dispatch(Modes{}, index_mode, [&](auto iv) {
          constexpr int D = decltype(dv)::value, IM = decltype(iv)::value;
          if constexpr (FI <= 64 || (D == 1 && IM == 1)) return launch_gather<FI, D, IM>(a);
          else return (int)GWEN_EINVAL;
        });
      });
    }
    return gwen::dispatch(Widths{}, F1, [&](auto fa) {
      return gwen::dispatch(gwen::ints<0, 16, 32, 64>{}, F2, [&](auto fb) {
        return gwen::dispatch(gwen::ints<0, 1>{}, pre != 0, [&](auto pv) {
          constexpr int FA = decltype(fa)::value, FB = decltype(fb)::value;
          constexpr bool PRE = decltype(pv)::value != 0;
          // activation-first has one contraction; a chained projection is the SHRINKING next layer's
          if constexpr (PRE ? FB == 0 : (FB > 0 && FB < FA)) {
            return gwen::dispatch(gwen::ints<2, 3>{}, gwen::images_of(contract), [&](auto nsv) {
              return gwen::dispatch(Depths{}, narrow(FI, FA) ? depth : 1, [&](auto dv) {   // depth 2: narrow only
                return gwen::dispatch(Modes{}, index_mode, [&](auto iv) {                  // records: narrow only
                  constexpr int NS = decltype(nsv)::value, D = decltype(dv)::value, IM = decltype(iv)::value;
                  // bf16x6 only where its three images fit a CU's LDS (gwen_gcn_chain_supported refuses the others)
                  if constexpr (Geom(FI, FA, FB, NS, 64).fits(kLdsCU) && ((D == 1 && IM == 1) || narrow(FI, FA))) {
                    if constexpr (narrow(FI, FA)) {
                      // the written-through kernels: at the depth and index mode the library launches for the shape
                      if constexpr (D == chain_depth(FI, FA, FB, NS) && IM == chain_index_mode(FI, FA, FB, PRE, NS)) {
                        if (store_mode == 3)
                          return packed == 2 ? launch_ns<FI, FA, FB, PRE, NS, D, IM, true, 3>(a, block_rows)
                                             : launch_ns<FI, FA, FB, PRE, NS, D, IM, false, 3>(a, block_rows);
                      }
                      if (store_mode != 1) return (int)GWEN_EINVAL;
                      if (packed == 2) return launch_ns<FI, FA, FB, PRE, NS, D, IM, true>(a, block_rows);
                    }
                    return launch_ns<FI, FA, FB, PRE, NS, D, IM>(a, block_rows);
                  } else {
                    return (int)GWEN_EINVAL;
                  }
                });
              });
            });
          } else {
            return (int)GWEN_EINVAL;
          }
        });
      });
    });
  });
}

extern "C" int gwen_gcn_chain_tuned4_f32(const int32_t *rowptr, const int32_t *col, const float *val,
                                         const float *x, const float *W1, const float *W2,
                                         const float *bias, float *out, int64_t N, int64_t Fin, int64_t F1,
                                         int64_t F2, int pre, int relu, int64_t members, int64_t mstride_x,
                                         int64_t mstride_o, int contract, int entries, int depth, int block_rows,
                                         int index_mode, const void *W1p, const void *W2p, int packed,
                                         gwen_stream_t stream_, int store_mode) {
  return chain_tuned(rowptr, col, val, x, W1, W2, bias, out, N, Fin, F1, F2, pre, relu, members, mstride_x, mstride_o,
                     contract, entries, depth, block_rows, index_mode, W1p, W2p, packed, store_mode, stream_, nullptr);
}

extern "C" int gwen_gcn_chain_tuned3_f32(const int32_t *rowptr, const int32_t *col, const float *val,
                                         const float *x, const float *W1, const float *W2,
                                         const float *bias, float *out, int64_t N, int64_t Fin, int64_t F1,
                                         int64_t F2, int pre, int relu, int64_t members, int64_t mstride_x,
                                         int64_t mstride_o, int contract, int entries, int depth, int block_rows,
                                         int index_mode, const void *W1p, const void *W2p, int packed,
                                         gwen_stream_t stream_) {
  return gwen_gcn_chain_tuned4_f32(rowptr, col, val, x, W1, W2, bias, out, N, Fin, F1, F2, pre, relu, members, mstride_x,
                                   mstride_o, contract, entries, depth, block_rows, index_mode, W1p, W2p, packed, stream_, 0);
}

extern "C" int gwen_gcn_chain_blocks_per_cu(const int32_t *rowptr, const int32_t *col, const float *val,
                                            const float *x, const float *W1, const float *W2,
                                            const float *bias, float *out, int64_t N, int64_t Fin, int64_t F1,
                                            int64_t F2, int pre, int relu, int64_t members, int64_t mstride_x,
                                            int64_t mstride_o, int contract, int entries, int depth, int block_rows,
                                            int index_mode, const void *W1p, const void *W2p, int packed,
                                            int *blocks_per_cu) {
  if (!blocks_per_cu || N <= 0 || members <= 0) return GWEN_EINVAL;
  return chain_tuned(rowptr, col, val, x, W1, W2, bias, out, N, Fin, F1, F2, pre, relu, members, mstride_x, mstride_o,
                     contract, entries, depth, block_rows, index_mode, W1p, W2p, packed, 0, nullptr, blocks_per_cu);
}

extern "C" int gwen_gcn_chain_tuned2_f32(const int32_t *rowptr, const int32_t *col, const float *val,
                                         const float *x, const float *W1, const float *W2,
                                         const float *bias, float *out, int64_t N, int64_t Fin, int64_t F1,
                                         int64_t F2, int pre, int relu, int64_t members, int64_t mstride_x,
                                         int64_t mstride_o, int contract, int entries, int depth, int block_rows,
                                         int index_mode, gwen_stream_t stream_) {
  return gwen_gcn_chain_tuned3_f32(rowptr, col, val, x, W1, W2, bias, out, N, Fin, F1, F2, pre, relu, members, mstride_x,
                                   mstride_o, contract, entries, depth, block_rows, index_mode, nullptr, nullptr, 0, stream_);
}

extern "C" int gwen_gcn_chain_tuned_f32(const int32_t *rowptr, const int32_t *col, const float *val,
                                        const float *x, const float *W1, const float *W2,
                                        const float *bias, float *out, int64_t N, int64_t Fin, int64_t F1,
                                        int64_t F2, int pre, int relu, int64_t members, int64_t mstride_x,
                                        int64_t mstride_o, int contract, int entries, int depth, int block_rows,
                                        gwen_stream_t stream_) {
  return gwen_gcn_chain_tuned2_f32(rowptr, col, val, x, W1, W2, bias, out, N, Fin, F1, F2, pre, relu, members,
                                   mstride_x, mstride_o, contract, entries, depth, block_rows, 0, stream_);
}

extern "C" int gwen_gcn_chain_entries_f32(const int32_t *rowptr, const int32_t *col, const float *val,
                                          const float *x, const float *W1, const float *W2,
                                          const float *bias, float *out, int64_t N, int64_t Fin, int64_t F1,
                                          int64_t F2, int pre, int relu, int64_t members, int64_t mstride_x,
                                          int64_t mstride_o, int contract, int entries, gwen_stream_t stream_) {
  return gwen_gcn_chain_tuned_f32(rowptr, col, val, x, W1, W2, bias, out, N, Fin, F1, F2, pre, relu, members,
                                  mstride_x, mstride_o, contract, entries, 0, 0, stream_);
}

extern "C" int gwen_gcn_chain_f32(const int32_t *rowptr, const int32_t *col, const float *val,
                                  const float *x, const float *W1, const float *W2,
                                  const float *bias, float *out, int64_t N, int64_t Fin, int64_t F1,
                                  int64_t F2, int pre, int relu, int64_t members, int64_t mstride_x,
                                  int64_t mstride_o, int contract, gwen_stream_t stream_) {
  return gwen_gcn_chain_entries_f32(rowptr, col, val, x, W1, W2, bias, out, N, Fin, F1, F2, pre, relu, members,
                                    mstride_x, mstride_o, contract, 8, stream_);
}
