// K4 -- one whole GCNConv layer (+ReLU) in a single launch, aggregate-first:
//            out = act( (A~ x) W^T + bias )
// Replaces, per layer of the reference, the sequence  lin (SGEMM) -> index_select -> mul ->
// scatter_add_ -> + bias -> relu  (torch-geometric 2.3.1 GCNConv.forward as called from
// /root/reference/src/gwen/models_gnn.py:147-149,:204-206) by ONE kernel: the [N,Fout] intermediate
// `h`, the [E',F] message tensor and four elementwise passes never touch HBM.
//
// Shape (wave64): many SHORT blocks -- K2's shape -- so that the waves sharing a SIMD are in
// different phases (gather / MFMA / store) and the per-wave critical path is one or two gathers:
//   block = NWB waves (one per 16-column output tile, at least 4) = BR consecutive destination rows;
//   phase 1  every wave gathers R = 64/(Fin/4) rows per pass (Fin/4 lanes per row, 16-B loads, the 8
//            entries of a group in flight together) from the GROUPED layout (rows padded to whole
//            groups of 8 with weight-0 entries, null group for absent rows), so every load in the
//            loop is unconditional -- a load under a per-lane condition makes hipcc branch around it
//            and wait vmcnt(0), which serialises the gathers.  On a uniform layout whose rows all hold
//            at most 7 entries (GE = 7, gather_rows.h) the 8th slot -- padding on every row -- is not
//            gathered at all.  The aggregated rows go to the block's
//            LDS tile.  Meanwhile each wave fetches ITS slice of W^T -- the B fragments of its 16
//            output columns -- straight from global memory (16 KB, L1/L2-resident) into registers.
//            "Meanwhile" is made true by hand in the narrow forward kernels (one chunk per block): the raw
//            W loads and the bias load (unconditional: from W itself and masked when there is no bias)
//            are issued first and nothing waits for them; the first column indices are requested right
//            behind them; W is split into its bf16 images in the shadow of the first pass's row loads
//            (gather_rows.h, shadow; pinned there: split.h, pin_here).  A block is then two dependent
//            round trips -- indices, rows -- where hipcc's own order was three: W and bias (vmcnt(0)),
//            the split, and only then the first index load, because the split is invariant in the chunk
//            loop that the narrow kernels shared with the persistent wide form and so sat above its
//            header.  The narrow forward now leaves that loop after its one chunk (no back edge); the
//            wide form and the backward compile to the code they had;
//   barrier;
//   phase 2  wave w owns output-column tile j = w % NJ of every (NWB/NJ)-th 16-row tile: A fragments
//            from LDS, MFMAs with W as the A operand (so the D tile comes out transposed: one lane =
//            4 consecutive output columns of one row), + bias, ReLU, one 16-B store per lane.
// Contraction (default): "3xbf16" -- x = hi + lo with hi = bf16(x), lo = bf16(x - hi), and
//   x.w ~= lo.hi' + hi.lo' + hi.hi' on v_mfma_f32_16x16x32_bf16 with fp32 accumulation; the dropped
//   lo.lo' term and the representation residual are < 2^-16 relative each (measured 8e-6 relative on
//   the 6-layer model; tolerance 1e-4).  The split is done once per element when the aggregated row
//   is written to LDS (hi and lo tiles, row pitch Fin/2+8 dwords => conflict-free 16-B reads).
//   It exists because the exact fp32 MFMA (1/16 of the bf16 rate) cost 7 of a 64->64 layer's 28 us.
// Contraction (exact = 2): "bf16x6" -- three images per operand, six MFMAs per k-step: 24 bits per operand, the
//   fp32-class default of the host API (split.h); one more LDS image of the tile.
// Contraction (exact = 1): v_mfma_f32_16x16x4_f32 on an fp32 tile (k-permutation k = 8q+2(lane>>4)+s,
//   row pitch Fin+4 floats => conflict-free 8-B reads): bit-exact fp32 fmaf chains.
// Blocks are remapped so that the blocks sharing an XCD (blockIdx % 8) own neighbouring rows.
// Stores (template argument ST, gather_rows.h store_out): the D tile leaves as one 16-byte store per lane, 16 rows x 64 B
//   per wave instruction.  ST = 1: plain stores.  ST = 3: the same instruction with the sc1 bit -- written through: the
//   line goes to memory at the store and leaves the XCD's L2, so the launch leaves no dirty output for its boundary to
//   write back (the next launch reads its input from beyond L2 either way).  Values, addresses, registers and LDS are
//   those of ST = 1.  Which shapes run 3: layer_store_mode (measured per kernel in the step, profiles/store_*).
//   Row stores (template argument RS, with ST = 3 only): the D tiles leave through an fp32 out tile in LDS as whole rows,
//   every wave instruction one run of 1024 / (4 Fout) consecutive rows -- one contiguous KiB where ldo == Fout.  The
//   wave holds its D tiles (bias and ReLU applied: the values of RS = false, bit for bit) until every wave of the block
//   is through its MFMAs; a barrier; the out tile is written OVER the images, which are dead by then; a second barrier;
//   the row stores, masked to rows < N at the store only.  The out tile has no pad: the 16-byte chunk c of row r lies
//   at chunk c ^ swz(r) of the row (out_chunk), which keeps the D-tile writes (8 consecutive rows, one chunk) and the
//   row reads (consecutive chunks) free of bank conflicts.  The row layout is this switch, orthogonal to the store
//   mode; mode numbers 2 / 4 of the C ABI stay reserved and refused.  Which shapes run it: layer_row_stores (measured
//   per kernel in the step, profiles/rowstore_*); the lab that priced it beforehand is tools/experiments/store_lab.patch.
#include "common.h"
#include "dispatch.h"
#include "gather_rows.h"
#include "split.h"

namespace {

constexpr int kTile = 16;
using gwen::bf16x4;
using gwen::bf16x8;
template <int K> using BF = gwen::BFv<K>;

// The block geometry of K4 -- the one copy of the rule.  Plain ints in, so the kernels read it at compile time (Cfg)
// and the extern "C" checks at run time (rows_ok).  ns: bf16 images per operand (2: bf16x3, 3: bf16x6, split.h); 0: the
// fp32-input MFMA.  brmin: rows per block asked for; a block is never less than one gather pass.
struct Geom {
  int G, R;                                                // lanes per gathered row, rows per wave pass
  int NJ, NWB;                                             // 16-column output tiles; waves per block: one per column tile
  int RB, BR;                                              // rows gathered per block pass, rows per block
  int PF, PB;                                              // tile row pitch: exact (floats), split (bf16)
  size_t lds_bytes;
  bool wide;                                               // the persistent form: one resident set of blocks walks the chunks
  constexpr Geom(int fin, int fout, int ns, int brmin)
      : G(fin / 4), R(64 / (fin / 4)), NJ(fout / 16), NWB(NJ > 8 ? 16 : (NJ > 4 ? 8 : 4)), RB(NWB * R),
        BR(RB > brmin ? RB : brmin), PF(fin + 4), PB(((fin / 2) % 16 == 8 ? fin / 2 : fin / 2 + 8) * 2),
        lds_bytes(ns > 0 ? (size_t)ns * BR * PB * 2 : (size_t)BR * PF * 4), wide(fin * fout >= 128 * 128) {}
};

template <int FIN, int FOUT, int NS, int BRMIN = 32>
struct Cfg {
  static constexpr Geom geo = Geom(FIN, FOUT, NS, BRMIN);
  static constexpr bool SPLIT = NS > 0;
  static constexpr int G = geo.G, R = geo.R, NJ = geo.NJ, NWB = geo.NWB, RB = geo.RB, BR = geo.BR;
  static constexpr int NP = BR / RB;                       // gather passes per wave
  static constexpr int NT = BR / kTile;                    // 16-row tiles per block
  static constexpr int TSTEP = NWB / NJ;                   // row tiles are strided over the waves
  static constexpr int NQ = FIN / 8;                       // exact: k-steps of 8
  static constexpr int KF = FIN >= 32 ? 8 : 4;             // split: bf16 per fragment (K = 32 or 16)
  static constexpr int KS = FIN / (4 * KF);                // split: MFMA k-steps
  static constexpr int PF = geo.PF, PB = geo.PB;
  static constexpr size_t lds_bytes = geo.lds_bytes;
  static_assert(NWB % NJ == 0, "waves must tile the output columns");
  static_assert(BR % RB == 0 && BR % kTile == 0, "a block is whole gather passes and whole row tiles");
};

// Row stores (k_layer's RS): the out tile of a block, [BR][Fout] fp32 with no pad, lies over the images; it is the larger
// of the two where the images are small (16 -> 32 at 64 rows: 8 192 B over 6 144).
constexpr size_t out_tile_bytes(size_t images, int br, int fout) {
  return images > (size_t)br * fout * 4 ? images : (size_t)br * fout * 4;
}

// Where the 16-byte chunk c of row r of the out tile lies, in chunks from the tile's start: chunk c ^ swz(r) of its row.
// Banks (64 x 4 B; a 16-byte write is served in groups of 8 consecutive lanes over 32 banks = 8 chunks, a 16-byte read in
// groups of 16 lanes over 64 banks = 16 chunks):
//   D-tile write: the 8 lanes of a group hold 8 consecutive rows (mi = 0 .. 7 or 8 .. 15) and ONE chunk c.  Rows are 16 / 8 /
//     4 chunks long (Fout = 64 / 32 / 16), so 8 chunks hold half a row, one row, two rows.  Fout >= 32: the 8 rows differ in
//     r & 7, so c ^ (r & 7) takes 8 different values mod 8.  Fout = 16: the four rows of one parity share their half of the
//     8 chunks and differ in (r >> 1) & 3, the two parities lie in the two halves.
//   row read: lane l reads chunk l % CR of row l / CR; a group is lanes {0-3, 12-15, 20-27} or {4-11, 16-19, 28-31} (+ 32).
//     Fout = 64: a group holds the chunk quads {0, 3} of an even row and {1, 2} of the odd row behind it (or the other way
//     round); r and r + 1 differ in bit 0 only, so the swizzle permutes the quads of both rows alike (bit 2 up) and
//     chunks inside a quad (bits 0, 1): the 16 chunks stay distinct.  Fout = 32: quads {0}, {1} of rows r, r + 1 and {1},
//     {0} of rows r + 2, r + 3 with r a multiple of 4; rows r and r + 2 share one half of the 16 chunks and bit 2 of the
//     swizzle, so their quads stay apart.  Fout = 16: four whole rows with four different r & 3: any permutation inside a
//     row keeps them apart.
template <int FOUT>
__device__ __forceinline__ int out_chunk(int r, int c) {
  constexpr int CR = FOUT / 4;
  const int swz = FOUT == 16 ? (r >> 1) & 3 : r & 7;
  return r * CR + (c ^ swz);
}

// Waves per SIMD asked of the register allocator for a row-store kernel; 0 = nothing is asked (no attribute is emitted, so
// every other kernel compiles as it did).  16 -> 32 on bf16x6 at 64 rows, 7 entries, W split in the kernel: left alone the
// row-store form takes 61 VGPRs + 4 AGPRs = 68 against 60 + 4, i.e. 7 blocks per CU where the kernel it replaces has 8;
// asked for 8 waves it takes 60 with the accumulator among them, no spill (profiles/rowstore_resource_usage.tsv).
constexpr int rs_waves(bool rs, int fin, int fout, int ns, int brmin, int ge, bool pk) {
  return rs && fin == 16 && fout == 32 && ns == 3 && brmin == 64 && ge == 7 && !pk ? 8 : 0;
}

// Which narrow forward shapes (Fin, Fout, images) run the two-round-trip prologue of the header: straight-line body,
// unconditional bias load, W split pinned in the shadow of the first row loads.  false keeps the order the kernel had
// (W and bias waited for and W split in front of the first index request), instruction for instruction.
// 16 -> 32 on bf16x6 stays as it was: the new order needs 61 VGPRs (+ 4 AGPRs) against 58, which is 7 waves per SIMD
// instead of 8, and measured no gain for it (9.19 -> 9.30 us, inside its spread; W is 4 floats per lane there).
constexpr bool layer_prologue(int fin, int fout, int ns) { return !(fin == 16 && fout == 32 && ns == 3); }

// BWD (the layer's backward, gwen_gcn_layer_bwd_f32): the aggregated rows are also stored (agg_out: the
// operand of grad_W) and the result is masked by mask > 0 (the ReLU of the layer below), so the launch
// returns the gradient the next backward launch starts from.
// GE: gathered entries per group (gather_rows.h); 7 only on the uniform layout.
// D: gather depth (gather_rows.h): passes of row loads a wave keeps in flight; the backward runs D = 1.
// IM: index mode (gather_rows.h): 2 = one record load per row and pass, broadcast in the lane group; narrow forward
// kernels on the uniform layout only.  Behind the older arguments, so that every other kernel keeps its name but for a ", 1".
// PK: packed W (packw.hip; narrow forward kernels on a bf16 split only): `W` points to the weight's bf16 images in fragment
// order, cut once per weight version, and this wave's B fragments are plain 16-byte loads at the top of the kernel -- no
// raw fp32 W, no split.  false compiles to the code the kernel had.
// ST: store mode of the epilogue (gather_rows.h, store_out): 1 = plain 16-byte stores, the code the kernel had; 3 = the same
// addresses written through (sc1).  Narrow forward kernels on the uniform layout and a bf16 split only.
// RS: row stores (the header, "Row stores"): the block's output leaves as whole rows through an out tile in LDS.  With
// ST = 3 only, so in the narrow forward, where a block has one chunk (the straight-line form, and 16 -> 32 on bf16x6
// without packed W, whose chunk loop runs once); false compiles to the code the kernel had.
template <int FIN, int FOUT, int NS, int BRMIN, bool UNI = false, bool BWD = false, int GE = 8, int D = 1, int IM = 1,
          bool PK = false, int ST = 1, bool RS = false>
__global__ __launch_bounds__((FOUT > 128 ? 1024 : (FOUT > 64 ? 512 : 256)))
__attribute__((amdgpu_waves_per_eu(rs_waves(RS, FIN, FOUT, NS, BRMIN, GE, PK)))) void k_layer(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const float *__restrict__ val, const float *__restrict__ x, const float *__restrict__ W,
    const float *__restrict__ bias, float *__restrict__ out, int32_t N, int64_t ldo,
    int64_t mstride_x, int64_t mstride_o, int relu, float *__restrict__ agg_out = nullptr,
    const float *__restrict__ mask = nullptr, float *__restrict__ bsum_out = nullptr, int32_t chunks_per_member = 0) {
  using C = Cfg<FIN, FOUT, NS, BRMIN>;
  static_assert(IM == 1 || (IM == 2 && UNI && !BWD && FIN <= 64 && FOUT <= 64), "index records: narrow forward, uniform layout");
  static_assert(!PK || (NS > 0 && !BWD && FIN <= 64 && FOUT <= 64), "packed W: narrow forward on a bf16 split");
  static_assert(ST == 1 || (ST == 3 && UNI && NS > 0 && !BWD && FIN <= 64 && FOUT <= 64), "store modes: narrow forward, uniform layout");
  static_assert(!RS || ST == 3, "row stores: with ST = 3 (narrow forward: one chunk per block, every thread at every barrier)");
  constexpr bool SPLIT = NS > 0;
  constexpr int NI = SPLIT ? NS : 1;
  __shared__ __attribute__((aligned(16))) char lds_raw[RS ? out_tile_bytes(C::lds_bytes, C::BR, FOUT) : C::lds_bytes];
  __shared__ float bred[BWD && FIN * FOUT < 128 * 128 ? 16 * 16 : 1];    // BWD, narrow: the waves' column sums of a chunk
  float *tile = reinterpret_cast<float *>(lds_raw);                      // exact: [BR][PF] fp32
  __bf16 *timg = reinterpret_cast<__bf16 *>(lds_raw);                    // split: NS images [BR][PB]
  constexpr int kImg = C::BR * C::PB;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int gl = lane % C::G, gr = lane / C::G;
  const int mi = lane & 15, mh = lane >> 4;

  // XCD-aware block remap (bijective for any grid size)
  const int nb = gridDim.x, bid = blockIdx.x;
  const int xcd = bid & 7, q8 = nb >> 3, r8 = nb & 7;
  const int lb = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);

  const char *xb = reinterpret_cast<const char *>(x + (int64_t)blockIdx.y * mstride_x);
  float *om = out + (int64_t)blockIdx.y * mstride_o;
  const uint32_t lane_off = gl * 16;                       // x rows are contiguous (ldx == Fin)

  // ---- this wave's B fragments (its 16 output columns of W^T), issued before the gathers ---------
  // Narrow forward kernels (one chunk per block, kShadow): only the RAW loads are issued here -- W, then bias, with no
  // wait behind them -- and the split into bf16 images waits for gather_passes' shadow, after the first pass's row
  // loads have left.  W then costs the block no round trip of its own: a block is indices, then rows.  The persistent
  // wide form and the backward keep the prologue they had: W split at once, above the chunk loop.
  constexpr bool kPersist = FIN * FOUT >= 128 * 128;
  constexpr bool kOnce = !kPersist && !BWD && (PK || layer_prologue(FIN, FOUT, NS));   // the narrow forward: one chunk per block
  constexpr bool kShadow = kOnce && SPLIT && !PK;
  const int j = wave % C::NJ;
  const float *wrow = W + (int64_t)(j * 16 + mi) * FIN;
  float2_t bfr[SPLIT ? 1 : C::NQ];
  typename BF<C::KF>::T bw[SPLIT ? C::KS : 1][NI];                       // W images per k-step
  float4_t wraw[kShadow ? C::KS : 1][kShadow ? C::KF / 4 : 1];   // kShadow: W as loaded
  if constexpr (PK) {
    // the images themselves, [j][ks][s][lane][KF]: one contiguous run per fragment, nothing to split
    using FT = typename BF<C::KF>::T;
    const __bf16 *wp = reinterpret_cast<const __bf16 *>(W) + ((int64_t)j * C::KS * NI * 64 + lane) * C::KF;
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks)
#pragma unroll
      for (int s_ = 0; s_ < NI; ++s_)
        bw[ks][s_] = *reinterpret_cast<const FT *>(wp + (ks * NI + s_) * 64 * C::KF);
  } else if constexpr (kShadow) {
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks)
#pragma unroll
      for (int i = 0; i < C::KF; i += 4)
        wraw[ks][i / 4] = *reinterpret_cast<const float4_t *>(wrow + C::KF * (4 * ks + mh) + i);
  } else if constexpr (SPLIT) {
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) {
      float wv[C::KF];
      const float *wp = wrow + C::KF * (4 * ks + mh);
#pragma unroll
      for (int i = 0; i < C::KF; i += 4) {
        const float4_t w4 = *reinterpret_cast<const float4_t *>(wp + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) wv[i + e] = w4[e];
      }
      gwen::split_images<C::KF, NI>(wv, bw[ks]);
    }
  } else {
#pragma unroll
    for (int q = 0; q < C::NQ; ++q)
      bfr[q] = *reinterpret_cast<const float2_t *>(wrow + 8 * q + 2 * mh);
  }
  float4_t bv4 = {0.f, 0.f, 0.f, 0.f};
  if constexpr (!kOnce) {
    if (bias) bv4 = *reinterpret_cast<const float4_t *>(bias + j * 16 + 4 * mh);
  } else {
    // never a load under a condition (gather_rows.h): without a bias the same 16 bytes of W are read (W holds
    // Fout * Fin >= Fout floats; packed: at least as many bytes) and masked to +0 -- the value bv4 has always had then --
    // in the shadow callable: masked here, the mask would wait for the load in front of the first index request
    bv4 = *reinterpret_cast<const float4_t *>((bias ? bias : W) + j * 16 + 4 * mh);
    __builtin_amdgcn_sched_barrier(0);                     // the raw loads stay in front of the first index request
  }
  auto split_w = [&]() {                                   // in the first row loads' shadow (kOnce)
    bv4 = gwen::masked_f4(bv4, bias != nullptr);
    gwen::pin_here(bv4);                                   // or mask and load sink to the epilogue
    if constexpr (PK) {                                    // the image loads stay at the top: their values are due here
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks)
#pragma unroll
        for (int s_ = 0; s_ < NI; ++s_) gwen::pin_here(bw[ks][s_]);
    }
    if constexpr (kShadow) {                               // raw W -> images
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) {
        float wv[C::KF];
#pragma unroll
        for (int i = 0; i < C::KF; i += 4)
#pragma unroll
          for (int e = 0; e < 4; ++e) wv[i + e] = wraw[ks][i / 4][e];
        gwen::split_images<C::KF, NI>(wv, bw[ks]);
#pragma unroll
        for (int s_ = 0; s_ < NI; ++s_) gwen::pin_here(bw[ks][s_]);   // or the optimiser sinks the split, and W's loads, to phase 2
      }
    }
  };

  // A block of the persistent wide form walks chunks lb, lb + grid, ... of BR rows: one resident set of blocks, so
  // that W -- fetched and split into this wave's registers once, above -- serves many chunks (at 256 channels W is
  // half as many bytes as a 64-row chunk gathers).  A narrow layer has one chunk per block; its forward leaves the
  // loop at the end of the body (if constexpr, below), so it is straight-line code: with a back edge the
  // (loop-invariant) W split had to sit above the loop header, in front of the gather.
  const int nchunks = kPersist ? (N + C::BR - 1) / C::BR : lb + 1;
  for (int chunk = lb; chunk < nchunks; chunk += nb) {
  const int b0 = chunk * C::BR;
  // ---- phase 1: gather + aggregate into the LDS tile (gather_rows.h) ------------------------------
  auto sink = [&](int lr, float4_t acc) {
        if constexpr (BWD) {
          if (agg_out && b0 + lr < N)
            *reinterpret_cast<float4_t *>(agg_out + (int64_t)blockIdx.y * mstride_x +
                                          (int64_t)(b0 + lr) * FIN + gl * 4) = acc;
        }
        if constexpr (SPLIT) {
          const float a4[4] = {acc[0], acc[1], acc[2], acc[3]};
          bf16x4 im[NI];
          gwen::split_images<4, NI>(a4, im);
#pragma unroll
          for (int s_ = 0; s_ < NI; ++s_)
            *reinterpret_cast<bf16x4 *>(timg + s_ * kImg + lr * C::PB + gl * 4) = im[s_];
        } else {
          *reinterpret_cast<float4_t *>(tile + lr * C::PF + gl * 4) = acc;
        }
      };
  if constexpr (kOnce)
    gwen::gather_passes<FIN, C::NP, C::RB, UNI, GE, D, IM>(rowptr, col, val, xb, N, b0, wave, gr, lane_off, sink, split_w);
  else
    gwen::gather_passes<FIN, C::NP, C::RB, UNI, GE, D, IM>(rowptr, col, val, xb, N, b0, wave, gr, lane_off, sink);
  __syncthreads();

  // ---- phase 2: (tile) x (this wave's 16 columns of W^T), bias, ReLU, store ----------------------
  if constexpr (RS) {
    // Row stores.  The arithmetic below is the loop's further down, statement for statement; only where o goes differs.
    constexpr int NTW = (C::NT + C::TSTEP - 1) / C::TSTEP;   // row tiles of a wave, at most
    float4_t ot[NTW];
#pragma unroll
    for (int k = 0; k < NTW; ++k) {
      const int tt = wave / C::NJ + k * C::TSTEP;
      if (C::NT % C::TSTEP == 0 || tt < C::NT) {             // wave-uniform
        f32x4 d = {0.f, 0.f, 0.f, 0.f};
        const int arow = (tt * kTile + mi) * C::PB;
#pragma unroll
        for (int ks = 0; ks < C::KS; ++ks) {
          using FT = typename BF<C::KF>::T;
          FT a[NI];
#pragma unroll
          for (int s_ = 0; s_ < NI; ++s_)
            a[s_] = *reinterpret_cast<const FT *>(timg + s_ * kImg + arow + C::KF * (4 * ks + mh));
          d = gwen::mma_split<C::KF, NI>(bw[ks], a, d);
        }
        float4_t o = float4_t{d[0], d[1], d[2], d[3]} + bv4;
        if (relu) {
#pragma unroll
          for (int t = 0; t < 4; ++t) o[t] = o[t] < 0.0f ? 0.0f : o[t];
        }
        ot[k] = o;
      }
    }
    __syncthreads();                                         // every wave is through with the images: the out tile goes over them
    float4_t *otile = reinterpret_cast<float4_t *>(lds_raw);   // [BR][FOUT / 4] chunks of 16 bytes, swizzled (out_chunk)
#pragma unroll
    for (int k = 0; k < NTW; ++k) {
      const int tt = wave / C::NJ + k * C::TSTEP;
      if (C::NT % C::TSTEP == 0 || tt < C::NT) otile[out_chunk<FOUT>(tt * kTile + mi, j * 4 + mh)] = ot[k];
    }
    __syncthreads();
    // wave instruction i: rows i RW .. i RW + RW - 1 of the block, lane l the l-th 16 bytes of that run of rows
    constexpr int CR = FOUT / 4, RW = 64 / CR, NINS = C::BR / RW;
    static_assert(C::BR % RW == 0, "a block is whole runs of rows");
    const int rr = lane / CR, rc = lane % CR;
#pragma unroll
    for (int i0 = 0; i0 < NINS; i0 += C::NWB) {
      const int i = i0 + wave;
      if (NINS % C::NWB == 0 || i < NINS) {                  // wave-uniform; no barrier follows
        const int lr = i * RW + rr;
        const float4_t o = otile[out_chunk<FOUT>(lr, rc)];
        if (b0 + lr < N) gwen::store_out<3>(om + (int64_t)(b0 + lr) * ldo + rc * 4, o);
      }
    }
    break;                                                   // kOnce: one chunk per block
  }
  float4_t cs = {0.f, 0.f, 0.f, 0.f};                  // BWD + bsum_out: this lane's column sums over the wave's row tiles
#pragma unroll
  for (int tt = wave / C::NJ; tt < C::NT; tt += C::TSTEP) {
    f32x4 d = {0.f, 0.f, 0.f, 0.f};
    if constexpr (SPLIT) {
      const int arow = (tt * kTile + mi) * C::PB;
#pragma unroll
      for (int ks = 0; ks < C::KS; ++ks) {
        using FT = typename BF<C::KF>::T;
        FT a[NI];
#pragma unroll
        for (int s_ = 0; s_ < NI; ++s_)
          a[s_] = *reinterpret_cast<const FT *>(timg + s_ * kImg + arow + C::KF * (4 * ks + mh));
        d = gwen::mma_split<C::KF, NI>(bw[ks], a, d);
      }
    } else {
      const float *ap = tile + (tt * kTile + mi) * C::PF + 2 * mh;
#pragma unroll
      for (int q = 0; q < C::NQ; ++q) {
        const float2_t a = *reinterpret_cast<const float2_t *>(ap + 8 * q);
        d = __builtin_amdgcn_mfma_f32_16x16x4f32(bfr[q][0], a[0], d, 0, 0, 0);
        d = __builtin_amdgcn_mfma_f32_16x16x4f32(bfr[q][1], a[1], d, 0, 0, 0);
      }
    }
    // W is the A operand, so D is the TRANSPOSED tile: lane (mi, mh) holds destination row mi,
    // output columns 16 j + 4 mh .. +3 -- one 16-B store per lane, 16 rows x 64 B per instruction
    const int r = b0 + tt * kTile + mi;
    float4_t o = float4_t{d[0], d[1], d[2], d[3]} + bv4;
    if (relu) {
#pragma unroll
      for (int t = 0; t < 4; ++t) o[t] = o[t] < 0.0f ? 0.0f : o[t];
    }
    if constexpr (BWD) {
      if (mask && r < N) {
        const float4_t y = *reinterpret_cast<const float4_t *>(mask + (int64_t)blockIdx.y * mstride_o +
                                                               (int64_t)r * ldo + j * 16 + 4 * mh);
#pragma unroll
        for (int t = 0; t < 4; ++t) o[t] = y[t] > 0.0f ? o[t] : 0.0f;
      }
    }
    if (r < N) gwen::store_out<ST>(om + (int64_t)r * ldo + j * 16 + 4 * mh, o);
    if constexpr (BWD && !kPersist) {
      if (bsum_out && r < N) cs = cs + o;
    }
  }
  if constexpr (BWD && !kPersist) {
    // the chunk's column sums of the masked result (= grad_b of the layer below, whose incoming gradient this is): rows
    // of a row tile meet through the 16 lanes that share mh, a column tile's waves through LDS in wave order; one
    // partial row per (member, chunk), every chunk written exactly once: fixed order, no atomics.  Narrow layers only
    // (one chunk per block): in the persistent wide kernels the extra registers cost more than the reduction launch
    // they replace (256 -> 256: 206 -> 289 us)
    if (bsum_out) {
#pragma unroll
      for (int m = 1; m < 16; m <<= 1)
#pragma unroll
        for (int t = 0; t < 4; ++t) cs[t] = cs[t] + __shfl_xor(cs[t], m);
      if (mi == 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t) bred[wave * 16 + 4 * mh + t] = cs[t];
      }
      __syncthreads();
      if ((int)threadIdx.x < FOUT) {
        const int cj = threadIdx.x >> 4, cc = threadIdx.x & 15;
        float v = 0.0f;
        for (int w = cj; w < C::NWB; w += C::NJ) v = v + bred[w * 16 + cc];
        bsum_out[((int64_t)blockIdx.y * chunks_per_member + chunk) * FOUT + threadIdx.x] = v;
      }
    }
  }
  if constexpr (kPersist) __syncthreads();     // the tile is free for the next chunk
  if constexpr (kOnce) break;                  // one chunk per block: no back edge
  }
}

// What one K4 launch works on; the forward and the backward entry points fill it once.
struct LayerArgs {
  const int32_t *rowptr, *col;                             // rowptr NULL = uniform layout
  const float *val, *x, *W, *bias;                         // W: the weight, or its packed images (launch_rows<.., PK>)
  float *out;
  int64_t N, ldo, members, msx, mso;
  int relu;
  hipStream_t st;
  float *agg_out; const float *mask; float *bsum_out; int64_t *chunks_out; bool bwd;   // the backward's: see k_layer
  int *probe;                                              // not NULL: launch nothing, store resident_blocks' blocks per CU
};

constexpr bool narrow(int fin, int fout) { return fin <= 64 && fout <= 64; }

// rows per block asked of the wide kernels: enough that W (read once per block) stays a small fraction of the gathered
// bytes; 256: 64 rows keep two blocks per CU in LDS (bf16x3), and 64 rows at 256 channels on bf16x6 as well
constexpr int wide_brmin(int fin) { return fin == 128 ? 128 : 64; }

// Rows per block of a packed-W kernel (PK) at gather depth 2 when no block size makes the grid co-resident, where that is
// not the 112 rows of the kernels that split W themselves; 0: the same.  64 -> 64 on bf16x6: 80 rows -- 38 400 B of LDS,
// so four blocks fit a CU where the 53 760 B of a 112-row block stop at three whatever the registers (116 VGPRs: four
// waves per SIMD) -- measured 14.5 us against 15.5 at 112 and 15.6 at 64 rows (profiles/packw_kernel_ab_*).
constexpr int packed_rows(int fin, int fout, int ns) { return fin == 64 && fout == 64 && ns == 3 ? 80 : 0; }

// Which rows per block exist for a shape: narrow layers 64 / 96 / 112 / 128 that are whole gather passes, wide layers
// the kernel's one size.  Decides which launch_rows are instantiated and what block_rows a caller may force.
// pk: the packed-W kernels also have 80 rows (Fin = 64: five passes) -- the largest block of 64 -> 64 on bf16x6 of which
// four fit a CU's LDS (38 400 B each; 96 rows and more: three).  Forced through block_rows, and the library's own fallback
// size where packed_rows() names it (launch()); never a candidate of the co-resident rule.
constexpr bool rows_ok(int fin, int fout, int br, bool pk = false) {
  if (!narrow(fin, fout)) return br == Geom(fin, fout, 0, wide_brmin(fin)).BR;
  return (br == 64 || (br == 80 && pk) || br == 96 || br == 112 || br == 128) && br % Geom(fin, fout, 0, br).RB == 0;
}

// Blocks of this instantiation that are resident at once.  Probed once per instantiation (function-local static): a warm
// call makes no HIP query, so the launchers stay capturable.  The UNIFORM kernel is probed whichever layout is launched:
// the block-rows choice of launch() on a non-uniform layout has always been made with the uniform kernel's occupancy.
// The index mode is part of the instantiation: a record kernel holds fewer registers.
template <int FIN, int FOUT, int NS, int BRMIN, int GE, int D, int IM, bool PK, int ST = 1, bool RS = false>
int resident_blocks(int64_t &resident) {
  static int per_cu = 0;
  if (per_cu == 0) {
    int nbk = 0;
    GWEN_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &nbk, reinterpret_cast<const void *>(&k_layer<FIN, FOUT, NS, BRMIN, true, false, GE, D, IM, PK, ST, RS>),
        Cfg<FIN, FOUT, NS, BRMIN>::NWB * 64, 0));
    per_cu = nbk < 1 ? 1 : nbk;
  }
  resident = (int64_t)256 * per_cu;
  return GWEN_OK;
}

template <int FIN, int FOUT, int NS, int BRMIN, int GE, int D, int IM, bool PK, int ST = 1, bool RS = false>
int launch_rows(const LayerArgs &a) {
  using C = Cfg<FIN, FOUT, NS, BRMIN>;
  int64_t resident = 0;
  { const int rc = resident_blocks<FIN, FOUT, NS, BRMIN, GE, D, IM, PK, ST, RS>(resident); if (rc != GWEN_OK) return rc; }
  if (a.probe) { *a.probe = (int)(resident / 256); return GWEN_OK; }
  int64_t blocks = (a.N + C::BR - 1) / C::BR;
  const int64_t chunks_pm = blocks;                        // chunks of BR rows per member (bsum_out: one partial row each)
  float *bsum_out = C::geo.wide ? nullptr : a.bsum_out;    // the persistent form: no fused column sums (see the kernel)
  if (a.chunks_out) *a.chunks_out = C::geo.wide ? 0 : chunks_pm * a.members;
  if (C::geo.wide && blocks > resident) blocks = resident; // wide layer: one resident set
  dim3 grid((unsigned)blocks, (unsigned)a.members);
  auto run = [&](auto kernel) {
    kernel<<<grid, C::NWB * 64, 0, a.st>>>(a.rowptr, a.col, a.val, a.x, a.W, a.bias, a.out, (int32_t)a.N, a.ldo, a.msx,
                                           a.mso, a.relu, a.agg_out, a.mask, bsum_out, (int32_t)chunks_pm);
    GWEN_LAUNCH_CHECK();
    return (int)GWEN_OK;
  };
  if constexpr (ST != 1) {                     // store modes: the forward on the uniform layout, nothing else
    if (a.bwd || a.rowptr) return GWEN_EINVAL;
    return run(&k_layer<FIN, FOUT, NS, BRMIN, true, false, GE, D, IM, PK, ST, RS>);
  } else if constexpr (IM == 2) {              // index records: the forward on the uniform layout, nothing else
    if (a.bwd || a.rowptr) return GWEN_EINVAL;
    return run(&k_layer<FIN, FOUT, NS, BRMIN, true, false, GE, D, 2, PK>);
  }
  if (a.bwd) {                                 // the backward runs on the layer's own split (bf16x3 / bf16x6), GE = 8, D = 1
    if constexpr ((NS == 2 || NS == 3) && GE == 8 && D == 1 && !PK)
      return a.rowptr ? run(&k_layer<FIN, FOUT, NS, BRMIN, false, true>) : run(&k_layer<FIN, FOUT, NS, BRMIN, true, true>);
    else
      return GWEN_EINVAL;
  }
  // uniform layout (no rowptr): row r is the group at 8 r; only there may the 8th slot go ungathered (GE = 7)
  return a.rowptr ? run(&k_layer<FIN, FOUT, NS, BRMIN, false, false, 8, D, 1, PK>)
                  : run(&k_layer<FIN, FOUT, NS, BRMIN, true, false, GE, D, 1, PK>);
}

// block_rows: 0 = the choice below; else forced (rows_ok, checked by the extern "C" caller)
template <int FIN, int FOUT, int NS, int GE, int D, int IM = 1, bool PK = false, int ST = 1, bool RS = false>
int launch(const LayerArgs &a, int block_rows) {
  static_assert(GE == 8 || narrow(FIN, FOUT), "7 gathered entries: narrow layers only");
  static_assert(IM == 1 || narrow(FIN, FOUT), "index records: narrow layers only");
  static_assert(D == 1 || narrow(FIN, FOUT), "gather depth 2: narrow layers only");
  static_assert(!PK || (narrow(FIN, FOUT) && NS > 0), "packed W: narrow layers on a bf16 split only");
  if constexpr (!narrow(FIN, FOUT)) {
    return launch_rows<FIN, FOUT, NS, wide_brmin(FIN), GE, D, 1, false>(a);
  } else {
    // f(BRV) for the block size br, where that size exists for this shape
    auto with_rows = [&](int br, auto &&f) {
      return gwen::dispatch(gwen::ints<64, 80, 96, 112, 128>{}, br, [&](auto brv) {
        if constexpr (rows_ok(FIN, FOUT, decltype(brv)::value, PK)) return f(brv);
        else return (int)GWEN_EINVAL;
      });
    };
    // Narrow layers run as ONE round of co-resident blocks when a block size makes that possible: with
    // 64-row blocks the c2 mesh needs 1 563 blocks against 1 024 resident ones (4 per CU at 64 -> 64),
    // i.e. a full round plus a half-empty one of ~10 us each; 112-row blocks (893 of them) fit one round.
    // Rows per block: 64 when that grid is co-resident or there are several members; else the smallest of 96 / 112 /
    // 128 (whole gather passes only) whose grid is co-resident; else 64 -- at gather depth 2 else 112 where the width
    // allows it: several rounds of blocks either way, and the two-deep gather fills and drains once per block, so the
    // longest run of passes is the cheapest (64 -> 64 on the c2 mesh, bf16x6: 18.2 us against 18.9 at 64 rows; depth 1
    // the other way round, 19.8 / 19.2).
    int rc = GWEN_OK, br = block_rows;
    auto fits = [&](int c, int64_t work) {                 // the grid of c-row blocks is co-resident (or rc says why not)
      int64_t res = 0;
      rc = with_rows(c, [&](auto brv) { return resident_blocks<FIN, FOUT, NS, decltype(brv)::value, GE, D, IM, PK, ST, RS>(res); });
      return rc != GWEN_OK || (work + c - 1) / c <= res;
    };
    if (br == 0) {
      br = D == 2 && rows_ok(FIN, FOUT, 112) ? 112 : 64;   // what is left when no size is co-resident
      if constexpr (PK && D == 2 && packed_rows(FIN, FOUT, NS) != 0) br = packed_rows(FIN, FOUT, NS);
      if (fits(64, a.N * a.members) || a.members > 1) {
        br = 64;
      } else {
        for (int c : {96, 112, 128})
          if (rows_ok(FIN, FOUT, c) && fits(c, a.N)) { br = c; break; }
      }
      if (rc != GWEN_OK) return rc;
    }
    return with_rows(br, [&](auto brv) { return launch_rows<FIN, FOUT, NS, decltype(brv)::value, GE, D, IM, PK, ST, RS>(a); });
  }
}

constexpr bool width_ok(int64_t f) { return f == 16 || f == 32 || f == 64 || f == 128 || f == 256; }

// f(FIN, FOUT, NS) as integral constants for a supported width pair and an image count of the list
template <int... NSs, class F>
int with_shape(int64_t Fin, int64_t Fout, gwen::ints<NSs...> images, int ns, F &&f) {
  using Widths = gwen::ints<16, 32, 64, 128, 256>;
  return gwen::dispatch(Widths{}, Fin, [&](auto fi) {
    return gwen::dispatch(Widths{}, Fout, [&](auto fo) {
      return gwen::dispatch(images, ns, [&](auto nsv) { return f(fi, fo, nsv); });
    });
  });
}

}  // namespace

extern "C" int gwen_gcn_layer_supported(int64_t Fin, int64_t Fout) {
  return width_ok(Fin) && width_ok(Fout) ? 1 : 0;
}

// The library's gather depth per (Fin, Fout, images) on the uniform layout: 2 only where the kernel measured
// faster on the MI355X ("Gather depth"; profiles/depth_*); the non-uniform layout and widths above 64 run
// depth 1.
static constexpr int layer_depth(int64_t fin, int64_t fout, int ns) {
  return fin == 64 && fout == 64 && ns == 3 ? 2 : 1;     // 64 -> 64 on bf16x6
}

extern "C" int gwen_gcn_layer_depth(int64_t Fin, int64_t Fout, int exact) {
  if (!gwen_gcn_layer_supported(Fin, Fout) || exact < 0 || exact > 2) return 0;
  if (!narrow(Fin, Fout)) return 1;
  return layer_depth(Fin, Fout, gwen::images_of(exact));
}

// The library's index mode per (Fin, Fout, images) on the uniform layout (gather_rows.h, IM): 2, one record load per row
// and pass, only where the kernel measured faster on the MI355X ("Index records"; profiles/index_*); the
// non-uniform layout, the backward and widths above 64 have mode 1 only.
static constexpr int layer_index_mode(int64_t fin, int64_t fout, int ns) {
  return (fin == 64 || fin == 32) && fout == 64 && ns == 3 ? 2 : 1;   // 64 -> 64 and 32 -> 64 on bf16x6
}

extern "C" int gwen_gcn_layer_index_mode(int64_t Fin, int64_t Fout, int exact) {
  if (!gwen_gcn_layer_supported(Fin, Fout) || exact < 0 || exact > 2) return 0;
  if (!narrow(Fin, Fout)) return 1;
  return layer_index_mode(Fin, Fout, gwen::images_of(exact));
}

// Whether the library's forward reads W as packed images (packw.hip; k_layer's PK) when the caller hands them over, per
// (Fin, Fout, images): on only where the kernel measured faster on the MI355X by the rule of the depth and index tables
// ("Packed W"; profiles/packw_*): 64 -> 64 on bf16x6 (16.7 -> 15.5 us at 112 rows).  32 -> 64 holds 92
// VGPRs against 72 with the images live across the gather and measured slower (11.9 -> 12.2 us), 16 -> 32 the same
// inside its spread (7.80 / 7.85): both keep the split in the kernel.
static constexpr bool layer_packed(int64_t fin, int64_t fout, int ns) { return fin == 64 && fout == 64 && ns == 3; }

extern "C" int gwen_gcn_layer_packed_mode(int64_t Fin, int64_t Fout, int exact) {
  if (!gwen_gcn_layer_supported(Fin, Fout) || exact < 0 || exact > 2) return 0;
  if (!narrow(Fin, Fout) || gwen::images_of(exact) == 0) return 1;
  return layer_packed(Fin, Fout, gwen::images_of(exact)) ? 2 : 1;
}

// The library's store mode per (Fin, Fout, images) on the uniform layout (gather_rows.h, store_out): 3, the epilogue's
// 16-byte stores written through, only where the kernel measured faster on the MI355X by the rule of the depth and index
// tables ("Stores"; profiles/store_*).  The modes exist for the narrow forward kernels on a bf16 split, on the
// uniform layout, at the shape's own depth and index mode; everything else has mode 1 only.
// The three K4 launches of the c2 step on bf16x6, the only split that was measured (profiles/store_kernel_ab.tsv).
static constexpr int layer_store_mode(int64_t fin, int64_t fout, int ns) {
  return ns == 3 && ((fin == 64 && fout == 64) || (fin == 32 && fout == 64) || (fin == 16 && fout == 32)) ? 3 : 1;
}

extern "C" int gwen_gcn_layer_store_mode(int64_t Fin, int64_t Fout, int exact) {
  if (!gwen_gcn_layer_supported(Fin, Fout) || exact < 0 || exact > 2) return 0;
  if (!narrow(Fin, Fout) || gwen::images_of(exact) == 0) return 1;
  return layer_store_mode(Fin, Fout, gwen::images_of(exact));
}

// Whether the library's written-through epilogue leaves as whole rows through an LDS out tile (k_layer's RS) per (Fin, Fout,
// images): on only where the launch measured faster in the step on the MI355X than the parent's launch, by more than the
// parent's per-launch standard deviation, in both of two profiled pairs ("Stores"; profiles/rowstore_*).
// Only bf16x6 with one member was measured.  Read only where the resolved store mode is 3.
// 32 -> 64 (11.23 -> 10.69 and 11.25 -> 10.75 us, parent's sd 0.29 / 0.32) and 16 -> 32 (6.68 -> 6.06 and 6.70 -> 6.05, sd 0.32 /
// 0.38) switch.  64 -> 64 does not: 13.43 -> 13.54 and 13.59 -> 13.61 -- five D tiles held over two barriers gain nothing at 80 rows.
static constexpr bool layer_row_stores(int64_t fin, int64_t fout, int ns) {
  return ns == 3 && ((fin == 32 && fout == 64) || (fin == 16 && fout == 32));
}

extern "C" int gwen_gcn_layer_row_stores(int64_t Fin, int64_t Fout, int exact) {
  if (!gwen_gcn_layer_supported(Fin, Fout) || exact < 0 || exact > 2) return 0;
  if (!narrow(Fin, Fout) || gwen::images_of(exact) == 0) return 1;
  const int ns = gwen::images_of(exact);
  return layer_store_mode(Fin, Fout, ns) == 3 && layer_row_stores(Fin, Fout, ns) ? 2 : 1;
}

// entries = 7: a promise of the caller (uniform layout, every row at most 7 stored entries) that the narrow
// kernels turn into one gather less per row; every other shape and layout gathers whole groups.
// depth, block_rows, index_mode: 0 = the library's choice (layer_depth; the co-resident grid of launch();
// layer_index_mode); none changes a value.  index_mode 1: every lane loads its row's group; 2: index records -- narrow
// layers on the uniform layout only, GWEN_EINVAL elsewhere
// Wp, packed: the gwen_gcn_packw_f32 images of W and whether they are read.  1: W is read and split in the kernel; 2: the
// images are read (W may be NULL) -- narrow layers on a bf16 split only, GWEN_EINVAL elsewhere or without images;
// 0: the library's choice -- the images where they are given and gwen_gcn_layer_packed_mode says 2.  No value changes.
// store_mode: 0 = the library's choice (layer_store_mode, one member only); 1 = plain stores; 3 = the same stores written
// through -- narrow layers on a bf16 split, on the uniform layout, at the library's depth and index mode for the shape,
// GWEN_EINVAL elsewhere; 2 and 4 are reserved numbers: GWEN_EINVAL.  No value changes.
// row_stores: how the written-through tile leaves (k_layer's RS).  1 = as the MFMA holds it, 16 rows x 64 B per wave
// instruction; 2 = as whole rows through an LDS out tile -- only where mode 3 is admitted and the resolved store mode is 3,
// GWEN_EINVAL elsewhere; 0 = the library's choice (layer_row_stores, one member and a resolved store mode of 3 only).  No
// value changes.
// probe: not NULL = launch nothing and store the blocks per CU that hipOccupancyMaxActiveBlocksPerMultiprocessor reports for
// the kernel this call would launch (the uniform-layout kernel, as resident_blocks has always asked)
static int layer_tuned(const int32_t *rowptr, const int32_t *col, const float *val,
                       const float *x, const float *W, const float *bias, float *out,
                       int64_t N, int64_t Fin, int64_t Fout, int64_t ldx, int64_t ldo,
                       int64_t members, int64_t mstride_x, int64_t mstride_o, int relu,
                       int exact, int entries, int depth, int block_rows, int index_mode,
                       const void *Wp, int packed, int store_mode, int row_stores, gwen_stream_t stream_, int *probe) {
  if (entries != 7 && entries != 8) return GWEN_EINVAL;
  if (store_mode < 0 || store_mode > 4) return GWEN_EINVAL;
  if (row_stores < 0 || row_stores > 2) return GWEN_EINVAL;
  if (packed < 0 || packed > 2) return GWEN_EINVAL;
  if (depth < 0 || depth > 2) return GWEN_EINVAL;
  if (index_mode < 0 || index_mode > 2) return GWEN_EINVAL;
  if (N < 0 || members < 0 || ldx < Fin || ldo < Fout || exact < 0 || exact > 2) return GWEN_EINVAL;
  if (!gwen_gcn_layer_supported(Fin, Fout)) return GWEN_EINVAL;
  if (index_mode == 2 && (rowptr || !narrow(Fin, Fout))) return GWEN_EINVAL;    // records: uniform layout, narrow layers
  // store modes: narrow layers on a bf16 split, uniform layout, the shape's own depth and index mode; 2 and 4: reserved
  const bool can_store = narrow(Fin, Fout) && gwen::images_of(exact) > 0 && !rowptr &&
                         (depth == 0 || depth == gwen_gcn_layer_depth(Fin, Fout, exact)) &&
                         (index_mode == 0 || index_mode == gwen_gcn_layer_index_mode(Fin, Fout, exact));
  if (store_mode > 1 && (!can_store || store_mode != 3)) return GWEN_EINVAL;
  if (store_mode == 0) store_mode = can_store && members == 1 ? gwen_gcn_layer_store_mode(Fin, Fout, exact) : 1;
  if (row_stores == 2 && store_mode != 3) return GWEN_EINVAL;                   // row stores: the written-through kernels only
  if (row_stores == 0)
    row_stores = store_mode == 3 && members == 1 && layer_row_stores(Fin, Fout, gwen::images_of(exact)) ? 2 : 1;
  const bool can_pack = narrow(Fin, Fout) && gwen::images_of(exact) > 0;        // packed W: narrow layers, bf16 splits
  if (packed == 2 && (!can_pack || !Wp)) return GWEN_EINVAL;
  if (packed == 0) packed = Wp && can_pack && gwen_gcn_layer_packed_mode(Fin, Fout, exact) == 2 ? 2 : 1;
  if (packed == 2 && !gwen_aligned(Wp, 16)) return GWEN_EINVAL;
  if (block_rows != 0 && !rows_ok(Fin, Fout, block_rows, packed == 2)) return GWEN_EINVAL;   // the one check of block_rows
  if (N == 0 || members == 0) return GWEN_OK;
  if (packed == 2 && !W) W = static_cast<const float *>(Wp);                     // never read then; the checks below hold
  if (!col || !val || !x || !W || !out || x == out) return GWEN_EINVAL;   // rowptr NULL = uniform
  if (N >= (int64_t(1) << 28) || members > 65535) return GWEN_ERANGE;     // 8 N must fit int32
  if (!gwen_aligned(x, 16) || !gwen_aligned(out, 16) || !gwen_aligned(W, 16) || ldx != Fin ||
      mstride_x % 4 || ldo % 4 || mstride_o % 4 || (bias && !gwen_aligned(bias, 16)))
    return GWEN_EINVAL;                       // x rows must be contiguous (32-bit row offsets)
  if (N * Fin * 4 >= (int64_t(1) << 32)) return GWEN_ERANGE;
  if (depth == 0) depth = rowptr ? 1 : gwen_gcn_layer_depth(Fin, Fout, exact);
  if (index_mode == 0) index_mode = rowptr ? 1 : gwen_gcn_layer_index_mode(Fin, Fout, exact);
  const int ge = entries == 7 && !rowptr ? 7 : 8;          // 7 on the uniform layout when the caller promises it
  const LayerArgs a{rowptr, col, val, x, packed == 2 ? static_cast<const float *>(Wp) : W, bias, out, N, ldo, members,
                    mstride_x, mstride_o, relu, gwen_stream(stream_), nullptr, nullptr, nullptr, nullptr, false, probe};
  return with_shape(Fin, Fout, gwen::ints<0, 2, 3>{}, gwen::images_of(exact), [&](auto fi, auto fo, auto nsv) {
    constexpr int FI = decltype(fi)::value, FO = decltype(fo)::value, NS = decltype(nsv)::value;
    if constexpr (narrow(FI, FO)) {            // narrow layers: GE x D x index mode x packed W
      return gwen::dispatch(gwen::ints<7, 8>{}, ge, [&](auto gev) {
        return gwen::dispatch(gwen::ints<1, 2>{}, depth, [&](auto dv) {
          return gwen::dispatch(gwen::ints<1, 2>{}, index_mode, [&](auto iv) {
            return gwen::dispatch(gwen::ints<1, 2>{}, packed, [&](auto pv) {
              constexpr bool PK = decltype(pv)::value == 2;
              constexpr int GE = decltype(gev)::value, D = decltype(dv)::value, IM = decltype(iv)::value;
              if constexpr (!PK || NS > 0) {
                // the written-through kernels: at the depth and index mode the library launches for the shape
                if constexpr (NS > 0 && D == layer_depth(FI, FO, NS) && IM == layer_index_mode(FI, FO, NS)) {
                  if (store_mode == 3)
                    return row_stores == 2 ? launch<FI, FO, NS, GE, D, IM, PK, 3, true>(a, block_rows)
                                           : launch<FI, FO, NS, GE, D, IM, PK, 3>(a, block_rows);
                }
                return store_mode == 1 ? launch<FI, FO, NS, GE, D, IM, PK>(a, block_rows) : (int)GWEN_EINVAL;
              } else {
                return (int)GWEN_EINVAL;
              }
            });
          });
        });
      });
    } else {                                   // the wide kernels gather whole groups at one depth
      return launch<FI, FO, NS, 8, 1>(a, block_rows);
    }
  });
}

extern "C" int gwen_gcn_layer_tuned5_f32(const int32_t *rowptr, const int32_t *col, const float *val,
                                         const float *x, const float *W, const float *bias, float *out,
                                         int64_t N, int64_t Fin, int64_t Fout, int64_t ldx, int64_t ldo,
                                         int64_t members, int64_t mstride_x, int64_t mstride_o, int relu,
                                         int exact, int entries, int depth, int block_rows, int index_mode,
                                         const void *Wp, int packed, gwen_stream_t stream_, int store_mode, int row_stores) {
  return layer_tuned(rowptr, col, val, x, W, bias, out, N, Fin, Fout, ldx, ldo, members, mstride_x, mstride_o, relu, exact,
                     entries, depth, block_rows, index_mode, Wp, packed, store_mode, row_stores, stream_, nullptr);
}

extern "C" int gwen_gcn_layer_tuned4_f32(const int32_t *rowptr, const int32_t *col, const float *val,
                                         const float *x, const float *W, const float *bias, float *out,
                                         int64_t N, int64_t Fin, int64_t Fout, int64_t ldx, int64_t ldo,
                                         int64_t members, int64_t mstride_x, int64_t mstride_o, int relu,
                                         int exact, int entries, int depth, int block_rows, int index_mode,
                                         const void *Wp, int packed, gwen_stream_t stream_, int store_mode) {
  return gwen_gcn_layer_tuned5_f32(rowptr, col, val, x, W, bias, out, N, Fin, Fout, ldx, ldo, members, mstride_x, mstride_o,
                                   relu, exact, entries, depth, block_rows, index_mode, Wp, packed, stream_, store_mode, 0);
}

extern "C" int gwen_gcn_layer_tuned3_f32(const int32_t *rowptr, const int32_t *col, const float *val,
                                         const float *x, const float *W, const float *bias, float *out,
                                         int64_t N, int64_t Fin, int64_t Fout, int64_t ldx, int64_t ldo,
                                         int64_t members, int64_t mstride_x, int64_t mstride_o, int relu,
                                         int exact, int entries, int depth, int block_rows, int index_mode,
                                         const void *Wp, int packed, gwen_stream_t stream_) {
  return gwen_gcn_layer_tuned4_f32(rowptr, col, val, x, W, bias, out, N, Fin, Fout, ldx, ldo, members, mstride_x, mstride_o,
                                   relu, exact, entries, depth, block_rows, index_mode, Wp, packed, stream_, 0);
}

extern "C" int gwen_gcn_layer_blocks_per_cu(const int32_t *rowptr, const int32_t *col, const float *val,
                                            const float *x, const float *W, const float *bias, float *out,
                                            int64_t N, int64_t Fin, int64_t Fout, int64_t ldx, int64_t ldo,
                                            int64_t members, int64_t mstride_x, int64_t mstride_o, int relu,
                                            int exact, int entries, int depth, int block_rows, int index_mode,
                                            const void *Wp, int packed, int *blocks_per_cu) {
  if (!blocks_per_cu || N <= 0 || members <= 0) return GWEN_EINVAL;
  return layer_tuned(rowptr, col, val, x, W, bias, out, N, Fin, Fout, ldx, ldo, members, mstride_x, mstride_o, relu, exact,
                     entries, depth, block_rows, index_mode, Wp, packed, 0, 0, nullptr, blocks_per_cu);
}

extern "C" int gwen_gcn_layer_tuned2_f32(const int32_t *rowptr, const int32_t *col, const float *val,
                                         const float *x, const float *W, const float *bias, float *out,
                                         int64_t N, int64_t Fin, int64_t Fout, int64_t ldx, int64_t ldo,
                                         int64_t members, int64_t mstride_x, int64_t mstride_o, int relu,
                                         int exact, int entries, int depth, int block_rows, int index_mode,
                                         gwen_stream_t stream_) {
  return gwen_gcn_layer_tuned3_f32(rowptr, col, val, x, W, bias, out, N, Fin, Fout, ldx, ldo, members, mstride_x,
                                   mstride_o, relu, exact, entries, depth, block_rows, index_mode, nullptr, 0, stream_);
}

extern "C" int gwen_gcn_layer_tuned_f32(const int32_t *rowptr, const int32_t *col, const float *val,
                                        const float *x, const float *W, const float *bias, float *out,
                                        int64_t N, int64_t Fin, int64_t Fout, int64_t ldx, int64_t ldo,
                                        int64_t members, int64_t mstride_x, int64_t mstride_o, int relu,
                                        int exact, int entries, int depth, int block_rows, gwen_stream_t stream_) {
  return gwen_gcn_layer_tuned2_f32(rowptr, col, val, x, W, bias, out, N, Fin, Fout, ldx, ldo, members, mstride_x,
                                   mstride_o, relu, exact, entries, depth, block_rows, 0, stream_);
}

extern "C" int gwen_gcn_layer_entries_f32(const int32_t *rowptr, const int32_t *col, const float *val,
                                          const float *x, const float *W, const float *bias, float *out,
                                          int64_t N, int64_t Fin, int64_t Fout, int64_t ldx, int64_t ldo,
                                          int64_t members, int64_t mstride_x, int64_t mstride_o, int relu,
                                          int exact, int entries, gwen_stream_t stream_) {
  return gwen_gcn_layer_tuned_f32(rowptr, col, val, x, W, bias, out, N, Fin, Fout, ldx, ldo, members, mstride_x,
                                  mstride_o, relu, exact, entries, 0, 0, stream_);
}

extern "C" int gwen_gcn_layer_f32(const int32_t *rowptr, const int32_t *col, const float *val,
                                  const float *x, const float *W, const float *bias, float *out,
                                  int64_t N, int64_t Fin, int64_t Fout, int64_t ldx, int64_t ldo,
                                  int64_t members, int64_t mstride_x, int64_t mstride_o, int relu,
                                  int exact, gwen_stream_t stream_) {
  return gwen_gcn_layer_entries_f32(rowptr, col, val, x, W, bias, out, N, Fin, Fout, ldx, ldo, members,
                                    mstride_x, mstride_o, relu, exact, 8, stream_);
}

// The layer's backward as ONE launch of the same kernel on the TRANSPOSED graph (grouped arrays of the
// transposed CSR):  gh = A~^T g  (stored: grad_W = gh^T x is a separate reduction),  gx = gh Wt^T  masked
// by mask > 0.  g [members, N, Fg]; Wt [Fx, Fg] = the layer's weight as stored ([out, in] = [Fg, Fx])
// TRANSPOSED; gh [members, N, Fg]; gx, mask [members, N, Fx] (mask NULL = no ReLU below).
// ... and, with bias_partial, the column sums of gx per (member, chunk of rows) as well: gx is the incoming gradient of
// the layer BELOW, so these are stage 1 of that layer's grad_b -- *bias_chunks partial rows of Fx floats (at most
// gwen_gcn_layer_bwd_bias_rows(N, members)), finished by gwen_reduce_chunks_batched.
extern "C" int64_t gwen_gcn_layer_bwd_bias_rows(int64_t N, int64_t members) { return members * ((N + 31) / 32); }

extern "C" int gwen_gcn_layer_bwd_bias_f32(const int32_t *t_rowptr, const int32_t *t_col, const float *t_val,
                                           const float *g, const float *Wt, const float *mask, float *gh,
                                           float *gx, int64_t N, int64_t Fg, int64_t Fx, int64_t members,
                                           int contract, float *bias_partial, int64_t *bias_chunks,
                                           gwen_stream_t stream_) {
  if (bias_chunks) *bias_chunks = 0;
  if (N < 0 || members < 0 || (contract != GWEN_CONTRACT_BF16X3 && contract != GWEN_CONTRACT_BF16X6)) return GWEN_EINVAL;
  if (!gwen_gcn_layer_supported(Fg, Fx)) return GWEN_EINVAL;
  if (N == 0 || members == 0) return GWEN_OK;
  if (!t_col || !t_val || !g || !Wt || !gx || g == gx) return GWEN_EINVAL;
  if (N >= (int64_t(1) << 28) || members > 65535) return GWEN_ERANGE;
  if (!gwen_aligned(g, 16) || !gwen_aligned(gx, 16) || !gwen_aligned(Wt, 16) ||
      (gh && !gwen_aligned(gh, 16)) || (mask && !gwen_aligned(mask, 16)))
    return GWEN_EINVAL;
  if (N * Fg * 4 >= (int64_t(1) << 32)) return GWEN_ERANGE;
  if ((bias_partial != nullptr) != (bias_chunks != nullptr) || (bias_partial && !gwen_aligned(bias_partial, 16))) return GWEN_EINVAL;
  const LayerArgs a{t_rowptr, t_col, t_val, g, Wt, nullptr, gx, N, Fx, members, N * Fg, N * Fx, 0, gwen_stream(stream_),
                    gh, mask, bias_partial, bias_chunks, true, nullptr};
  return with_shape(Fg, Fx, gwen::ints<2, 3>{}, gwen::images_of(contract), [&](auto fi, auto fo, auto nsv) {
    return launch<decltype(fi)::value, decltype(fo)::value, decltype(nsv)::value, 8, 1>(a, 0);
  });
}

extern "C" int gwen_gcn_layer_bwd_f32(const int32_t *t_rowptr, const int32_t *t_col, const float *t_val,
                                      const float *g, const float *Wt, const float *mask, float *gh,
                                      float *gx, int64_t N, int64_t Fg, int64_t Fx, int64_t members,
                                      int contract, gwen_stream_t stream_) {
  return gwen_gcn_layer_bwd_bias_f32(t_rowptr, t_col, t_val, g, Wt, mask, gh, gx, N, Fg, Fx, members, contract, nullptr,
                                     nullptr, stream_);
}
