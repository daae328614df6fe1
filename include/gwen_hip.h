/*
 * gwen_hip.h -- C ABI of libgwen_hip.so: the MI355X (gfx950) implementation of GWEN's GCNConv
 * hot path.  Plain pointers and sizes only; no torch types.  Every pointer is a DEVICE pointer
 * unless the comment says "host".  All launchers are asynchronous on `stream` (a hipStream_t
 * passed as void*), allocate nothing, synchronise nothing and keep no global state, so they can be
 * captured into a hipGraph.
 *
 * The reference (MeteoSwiss/GWEN) has no C/FFI layer: its hot path is the Python call
 * `GCNConv.__call__(x, edge_index)` into torch-geometric 2.3.1
 * (/root/reference/src/gwen/models_gnn.py:19 import; :118-130,:172-184 constructors;
 * :147-149,:204-206 calls).  Each entry point below names the piece of that call it replaces.
 * The Python binding a maintainer adds is shown in INTEGRATION.md.
 *
 * Return value: 0 on success; > 0 a hipError_t; < 0 one of the GWEN_E* codes.
 */
#ifndef GWEN_HIP_H
#define GWEN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GWEN_OK 0
#define GWEN_EINVAL (-1)    /* bad size / null pointer / misaligned argument            */
#define GWEN_ERANGE (-2)    /* N, E or a byte count does not fit the int32 CSR          */
#define GWEN_ENOSPACE (-3)  /* workspace smaller than gwen_gcn_prep_workspace_bytes()   */

typedef void *gwen_stream_t; /* hipStream_t */

/* Library identification: "gwen_hip <semver> gfx950". */
const char *gwen_hip_version(void);
/* Text for a return code of any function below (hipGetErrorString for positive codes). */
const char *gwen_hip_error_string(int code);

/* ---------------------------------------------------------------------------------------------
 * K1  graph preparation == gcn_norm + add_remaining_self_loops, hoisted out of the layer
 * (the reference recomputes it inside each of the 6 GCNConv calls of every forward:
 *  /root/reference/src/gwen/models_gnn.py:147-149,:204-206; constructors pass cached=False).
 *
 * edge_index : int64 [2, E] row-major; row 0 = source j, row 1 = target i.
 * edge_weight: fp32 [E] or NULL (unit weights; the reference never passes weights).
 * Result: CSR by TARGET node with the N self-loops completed,
 *   rowptr int32 [N+1], col int32 [cap], val fp32 [cap], eid int32 [cap], cap = E + N,
 *   where row i holds its kept (non-loop) in-edges in ORIGINAL edge order followed by the
 *   self-loop -- the order in which the reference's CPU scatter-add visits them --
 *   col = source node, val = d^-1/2[src] * w * d^-1/2[dst] (or the raw w if !normalize),
 *   eid = index of the edge in edge_index, -1 for a completed self-loop.
 *   dis fp32 [N] = deg^-1/2 (inf -> 0).  rowptr[N] = number of stored entries E'.
 * status: int32 [2]; status[0] is OR-ed with 1 if any node index is outside [0, N)
 *   (such edges are dropped); status[1] = E'.  The caller zeroes nothing: prep does.
 * ------------------------------------------------------------------------------------------- */
int gwen_gcn_prep_workspace_bytes(int64_t N, int64_t E, size_t *bytes /* host */);
int gwen_gcn_prep(const int64_t *edge_index, const float *edge_weight, int64_t N, int64_t E,
                  int add_self_loops, float fill_value, int normalize, int32_t *rowptr,
                  int32_t *col, float *val, int32_t *eid, float *dis, int32_t *status,
                  void *workspace, size_t workspace_bytes, gwen_stream_t stream);

/* Rectangular (bipartite) graph for the grid->mesh / mesh->grid maps of SURVEY 8(f) f2 (BUILD-DEFINED:
 * the reference has no such graphs): edges run from N_src source nodes to N_dst target
 * nodes, no self-loops; CSR by target as above with rowptr [N_dst+1].  mean = 1: val = w / (sum of the
 * row's weights) (mean aggregation); mean = 0: val = w.  K2/K4 take it as is (x has N_src rows).
 * workspace: gwen_gcn_prep_workspace_bytes(N_dst, E). */
int gwen_gcn_prep_rect(const int64_t *edge_index, const float *edge_weight, int64_t N_src,
                       int64_t N_dst, int64_t E, int mean, int32_t *rowptr, int32_t *col, float *val,
                       int32_t *eid, int32_t *status, void *workspace, size_t workspace_bytes,
                       gwen_stream_t stream);

/* Transposed structure (CSR by SOURCE) of a prepared graph, for the backward pass
 * (grad_h = A~^T grad_out).  Same value array semantics; rows keep target order ascending.
 * workspace: same size as for gwen_gcn_prep with E := rowptr[N] upper bound (E + N). */
int gwen_gcn_transpose(const int32_t *rowptr, const int32_t *col, const float *val, int64_t N,
                       int64_t cap, int32_t *t_rowptr, int32_t *t_col, float *t_val,
                       void *workspace, size_t workspace_bytes, gwen_stream_t stream);
/* The same for a rectangular CSR (gwen_gcn_prep_rect: N target rows, columns in [0, N_t)): the transpose
 * has N_t rows (t_rowptr [N_t + 1]).  workspace: gwen_gcn_prep_workspace_bytes(max(N, N_t), cap). */
int gwen_gcn_transpose_rect(const int32_t *rowptr, const int32_t *col, const float *val, int64_t N,
                            int64_t N_t, int64_t cap, int32_t *t_rowptr, int32_t *t_col, float *t_val,
                            void *workspace, size_t workspace_bytes, gwen_stream_t stream);

/* Grouped layout of a prepared graph for K4: every row padded to a whole number of 8-entry groups
 * (padding entries carry weight 0 and the column of the row's first entry), so the kernel reads
 * indices and weights as aligned 32-byte groups and needs no per-entry bounds logic.
 *   g_rowptr int32 [N+1] (entry offsets, multiples of 8), g_col / g_val [gwen_gcn_group8_capacity()],
 *   followed at g_rowptr[N] by one all-zero "null group" (col 0, weight 0).
 * uniform (int32 [1], may be NULL) is set to 1 when EVERY row is exactly one group (bounded-degree
 *   meshes: 1 <= entries <= 8), i.e. g_rowptr[r] == 8 r.  K4/K5 then accept rowptr == NULL and skip the
 *   row-pointer lookup (one dependent load less per gathered row).
 * workspace: as for gwen_gcn_prep. */
int64_t gwen_gcn_group8_capacity(int64_t N, int64_t cap);
int gwen_gcn_group8(const int32_t *rowptr, const int32_t *col, const float *val, int64_t N,
                    int64_t cap, int32_t *g_rowptr, int32_t *g_col, float *g_val, int32_t *uniform,
                    void *workspace, size_t workspace_bytes, gwen_stream_t stream);
/* The bound of a prepared CSR: *max_entries (device int32 [1]) = the largest number of stored entries of any row
 * (0 for N = 0).  One small launch, no atomics; read it back once per graph, with `uniform`.  On a uniform layout
 * whose bound is at most 7 -- a geodesic mesh: 6 neighbours and the self loop -- slot 7 of every group is padding,
 * and the *_entries_f32 forms of K4 / K5 / the stack launcher may be told entries = 7. */
int gwen_gcn_max_entries(const int32_t *rowptr, int64_t N, int32_t *max_entries, gwen_stream_t stream);

/* Content checksum of a device buffer (128 bits: two independent position-dependent 64-bit sums over its
 * 8-byte words), the key under which a caller caches prepared graphs: the reference's loaders hand every
 * forward a NEW edge_index tensor with the same edges (/root/reference/src/gwen/models_gnn.py:351-360).
 * data: 8-byte aligned; out: uint64 [2] (device); workspace: gwen_checksum_workspace_bytes() bytes.
 * Deterministic; two small launches; nothing is read back here. */
int64_t gwen_checksum_workspace_bytes(void);
int gwen_checksum128(const void *data, int64_t bytes, uint64_t *out, void *workspace,
                     int64_t workspace_bytes, gwen_stream_t stream);

/* Row segmentation for LONG rows (graphs beyond K7's 256 nodes whose rows are much longer than the 8 entries
 * one lane group gathers per round trip: complete graphs over more than 256 members, hub nodes).  Row r of
 * the CSR (length len) is cut into max(1, ceil(len / S)) segments of S entries:
 *     seg_rowptr int32 [n_seg + 1]   a REFINEMENT of rowptr over the same col / val arrays: K2 on
 *                                    (seg_rowptr, col, val) gives one partial sum per segment, every segment
 *                                    summed in stored order by its own lane group (edge-parallel);
 *     rowptr2 [N + 1], col2 = 0 .. n_seg - 1, val2 = 1   the CSR that adds each row's partial sums in
 *                                    segment order: K2 on it (bias / ReLU there) finishes the row.
 * Deterministic (fixed order, no atomics); differs from K2's sequential sum by rounding order only.
 * rowptr2 itself may be segmented again when a row has more than S segments.
 * status int32 [2]: [0] = most segments of a row, [1] = longest row.  n_seg = rowptr2[N] <=
 * gwen_gcn_segments_capacity(N, nnz, S).  workspace: gwen_gcn_prep_workspace_bytes(N, 0) bytes. */
int64_t gwen_gcn_segments_capacity(int64_t N, int64_t nnz, int64_t S);
int gwen_gcn_segments(const int32_t *rowptr, int64_t N, int64_t S, int32_t *rowptr2, int32_t *seg_rowptr,
                      int32_t *col2, float *val2, int32_t *status, void *workspace,
                      size_t workspace_bytes, gwen_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K2  fused propagate == MessagePassing.propagate (message w~ * x_j, aggregate add at target)
 *     + bias add (GCNConv.forward) + torch.relu (/root/reference/src/gwen/models_gnn.py:147-149,
 *     :204-205) in one pass:   out[m,i,:] = act( sum_s val[s] * h[m, col[s], :] + bias ).
 * h   : fp32 [members, N, F] with row stride ldh (>= F) and member stride mstride_h (elements).
 * out : fp32 [members, N, F] with row stride ldo and member stride mstride_o.  out != h.
 * bias: fp32 [F] or NULL.  relu: 0/1.
 * Terms are added sequentially in stored order with a rounded product per term (no FMA), so the
 * result is bitwise reproducible and equals a sequential CPU scatter-add in edge order.
 *
 * PITCHES AND MEMBER STRIDES, here and in every entry point below that takes an ld* or an mstride_* (all in
 * elements): cell (m, r, c) of an operand is at base + m * mstride + r * ld + c.  An operand of `rows` rows of F
 * elements at pitch ld (>= F) needs (rows - 1) * ld + F elements, and (members - 1) * mstride more for its members:
 * nothing behind the last logical cell is read into a result or written, and no output cell outside the logical ones
 * is written (row padding, gaps between members).  Members may interleave (mstride < rows * ld, e.g. ld = members * F,
 * mstride = F) as long as no two logical cells coincide.  Entry points without an ld take contiguous rows (ld = F).
 * K2 takes any pitch and base (vectors of 4 / 2 / 1 floats by what divides F, the pitches, the strides and the
 * addresses); the kernels that move 16-byte vectors (K4, K5, K7, K8) say so and refuse other values with GWEN_EINVAL.
 * ------------------------------------------------------------------------------------------- */
int gwen_gcn_propagate_f32(const int32_t *rowptr, const int32_t *col, const float *val,
                           const float *h, const float *bias, float *out, int64_t N, int64_t F,
                           int64_t ldh, int64_t ldo, int64_t members, int64_t mstride_h,
                           int64_t mstride_o, int relu, gwen_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Contractions.  The reference's `lin` is an fp32 GEMM (/root/reference/src/gwen/models_gnn.py:118-130 -> PyG
 * Linear).  Every kernel with a dense contraction (K3, K4, K5, K8) takes one of these codes (the parameter is
 * called `exact` in K3 / K4 for history, `contract` elsewhere):
 *   GWEN_CONTRACT_BF16X3 (0)  operands cut into two bf16 images (x = hi + lo), 3 MFMAs per k-step, fp32
 *                             accumulation: ~17 bits per product, 7e-6 relative on the 6-layer model;
 *   GWEN_CONTRACT_F32    (1)  fp32-input MFMA: bit-identical to a k-ordered fp32 fmaf chain, 1/16 of the bf16 rate;
 *   GWEN_CONTRACT_BF16X6 (2)  three bf16 images per operand, 6 MFMAs per k-step: 24 bits per operand, fp32-class
 *                             (<= 2e-6 on the 6-layer model) at 6/16 of the fp32 MFMA's cost;
 *   GWEN_CONTRACT_F16X3  (3)  two fp16 images per operand, both operands scaled by exact powers of two (W per output
 *                             column, the rows per 64-feature chunk) so that fp16's range holds them: operands kept to
 *                             2^-24, 3 MFMAs per k-step -- fp32-class at bf16x3's cost.  K8 has it at every
 *                             width (gwen_gcn_wide_layer_f32).  On a layer of the stack launcher
 *                             (gwen_layer_desc.contract) it means "fp32-class on the kernel's own split": K8 runs
 *                             f16x3, K3 / K4 / K5 / K7 run bf16x6 -- the host API's default.
 * ------------------------------------------------------------------------------------------- */
#define GWEN_CONTRACT_BF16X3 0
#define GWEN_CONTRACT_F32 1
#define GWEN_CONTRACT_BF16X6 2
#define GWEN_CONTRACT_F16X3 3

/* ---------------------------------------------------------------------------------------------
 * K3  dense projection == GCNConv.lin (PyG Linear(Fin, Fout, bias=False)):  h = x @ W^T.
 * x [rows, Fin] (row stride ldx), W [Fout, Fin] contiguous (lin.weight), h [rows, Fout]
 * (row stride ldh).  Optional epilogue: + bias[Fout] (NULL = none), ReLU.
 * exact: a GWEN_CONTRACT_* code (0: bf16x3 split, fp32 accumulate, as K4; 1: fp32-input MFMA
 *   v_mfma_f32_32x32x2_f32, bit-identical to a k-ordered fp32 fmaf chain; 2: bf16x6 split).
 * workspace (optional, gwen_gcn_linear_workspace_floats() elements; 0 = not needed): lets the split
 *   variant cut a long K over several blocks when there are few output tiles (few rows x wide input,
 *   the reference's own C -> 1024 projection on ~125 nodes) and add the partial products in a fixed
 *   order; without it that shape runs on a handful of CUs.
 * ------------------------------------------------------------------------------------------- */
int64_t gwen_gcn_linear_workspace_floats(int64_t rows, int64_t Fin, int64_t Fout);
int gwen_gcn_linear_f32(const float *x, const float *W, const float *bias, float *h, int64_t rows,
                        int64_t Fin, int64_t Fout, int64_t ldx, int64_t ldh, int relu, int exact,
                        float *workspace, int64_t workspace_floats, gwen_stream_t stream);
/* The same product with the weight operand given as Wt [Fin, Fout] row-major ("NN"): h = act(x Wt + bias).  The
 * backward's gx = gh W with W as the layer stores it ([out, in] of the forward = [K, N] here), without a transposing
 * copy; out = D g for a dense adjacency D.  Split contractions only (GWEN_CONTRACT_BF16X3 / BF16X6; F16X3 = BF16X6
 * here), ldw == Fout, x != h; workspace as gwen_gcn_linear_f32 (split-K). */
int gwen_gcn_linear_nn_f32(const float *x, const float *Wt, const float *bias, float *h, int64_t rows, int64_t Fin,
                           int64_t Fout, int64_t ldx, int64_t ldw, int64_t ldh, int relu, int contract,
                           float *workspace, int64_t workspace_floats, gwen_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K4  one whole GCNConv layer (+ReLU) in a single launch, aggregate-first:
 *        out = act( (A~ x) W^T + bias )        (== A~ (x W^T) + bias, A~ linear)
 * Gathers x at width Fin, keeps the aggregated tile in LDS, contracts it with W on the matrix cores
 * and stores once at width Fout: no [N, Fout] intermediate `h` goes through HBM.
 * exact = 0: the contraction runs as a 3-term bf16 split (x = hi + lo, fp32 accumulate; < 2^-15
 *   relative per product, 8e-6 measured on the 6-layer model against a 1e-4 tolerance);
 * exact = 1: fp32-input MFMA, bit-exact fp32 fmaf chains (about 1.3x slower at 64 -> 64);
 * exact = 2: bf16x6 split (GWEN_CONTRACT_BF16X6), one more LDS image of the tile.
 * rowptr/col/val here are the GROUPED arrays of gwen_gcn_group8() (rows in whole groups of 8, null
 * group at rowptr[N]; rowptr may be NULL for a uniform layout, see gwen_gcn_group8); x rows must be contiguous (ldx == Fin) and N * Fin * 4 < 2^32.
 * Supported widths: Fin, Fout in {16, 32, 64, 128, 256} (gwen_gcn_layer_supported() says; otherwise
 * GWEN_EINVAL: use K3 + K2).  Same alignment rules as K2.
 * ------------------------------------------------------------------------------------------- */
int gwen_gcn_layer_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *x,
                       const float *W, const float *bias, float *out, int64_t N, int64_t Fin,
                       int64_t Fout, int64_t ldx, int64_t ldo, int64_t members, int64_t mstride_x,
                       int64_t mstride_o, int relu, int exact, gwen_stream_t stream);
int gwen_gcn_layer_supported(int64_t Fin, int64_t Fout);
/* The same with the number of entries of a group that are gathered: entries = 8 is gwen_gcn_layer_f32; entries = 7
 * is the CALLER'S PROMISE that rowptr is NULL (uniform layout) and that every row holds at most 7 stored entries
 * (gwen_gcn_max_entries), like the `uniform` contract itself: on a graph with a row of 8 the 8th entry is silently
 * dropped.  Fin, Fout <= 64 then issue 7 row gathers and 7 FMA groups per row instead of 8; with a non-NULL rowptr or at
 * other widths the whole group is gathered.  For finite inputs every value equals that of entries = 8 (the skipped
 * term is fma(0, v, acc)); only the sign of an exact zero can differ, and an Inf / NaN in the row of a destination's
 * first entry (the padding slot's column) is no longer turned into NaN through 0 * Inf.  entries outside {7, 8}:
 * GWEN_EINVAL. */
int gwen_gcn_layer_entries_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *x,
                               const float *W, const float *bias, float *out, int64_t N, int64_t Fin,
                               int64_t Fout, int64_t ldx, int64_t ldo, int64_t members, int64_t mstride_x,
                               int64_t mstride_o, int relu, int exact, int entries, gwen_stream_t stream);
/* The same with two scheduling choices of the narrow kernels (Fin, Fout <= 64) exposed, for tests and A/B timing.
 * NEITHER CHANGES A VALUE: every output is bitwise that of gwen_gcn_layer_entries_f32, which forwards with 0, 0.
 * depth: passes of row loads a wave keeps in flight while it gathers -- 1, 2, or 0 = the library's choice
 *   (gwen_gcn_layer_depth on a uniform layout, 1 with a row pointer).  Widths above 64 always run depth 1.
 * block_rows: destination rows per block -- 0 = the library's choice (the smallest of 64 / 96 / 112 / 128 whose grid
 *   is co-resident; if none is, 64 at depth 1 and 112 at depth 2), or one of these that is a whole number of gather passes (16 * 64 / Fin rows for Fout <= 64:
 *   all four at Fin = 64; 64, 96, 128 at Fin = 32; 64, 128 at Fin = 16); widths above 64: 0 or the kernel's one size.
 * depth outside {0, 1, 2} or any other block_rows: GWEN_EINVAL. */
int gwen_gcn_layer_tuned_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *x,
                             const float *W, const float *bias, float *out, int64_t N, int64_t Fin,
                             int64_t Fout, int64_t ldx, int64_t ldo, int64_t members, int64_t mstride_x,
                             int64_t mstride_o, int relu, int exact, int entries, int depth, int block_rows,
                             gwen_stream_t stream);
/* the depth gwen_gcn_layer_f32 runs on a uniform layout: 1 or 2 (0: unsupported widths / exact) */
int gwen_gcn_layer_depth(int64_t Fin, int64_t Fout, int exact);
/* gwen_gcn_layer_tuned_f32 with a third scheduling choice that CHANGES NO VALUE (every output is bitwise the same,
 * signed zeros included); gwen_gcn_layer_tuned_f32 forwards with 0.
 * index_mode: how the lanes that share a destination row get its column indices and weights -- 1 = every lane loads
 *   the row's whole group of 8 + 8; 2 = "index records": each lane loads its share of the 64 bytes once per row and the
 *   values are broadcast inside the lane group (Fin, Fout <= 64 on the uniform layout only: with a row pointer or at
 *   other widths GWEN_EINVAL); 0 = the library's choice (gwen_gcn_layer_index_mode on a uniform layout, else 1).
 * index_mode outside {0, 1, 2}: GWEN_EINVAL. */
int gwen_gcn_layer_tuned2_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *x,
                              const float *W, const float *bias, float *out, int64_t N, int64_t Fin,
                              int64_t Fout, int64_t ldx, int64_t ldo, int64_t members, int64_t mstride_x,
                              int64_t mstride_o, int relu, int exact, int entries, int depth, int block_rows,
                              int index_mode, gwen_stream_t stream);
/* the index mode gwen_gcn_layer_f32 runs on a uniform layout: 1 or 2 (0: unsupported widths / exact) */
int gwen_gcn_layer_index_mode(int64_t Fin, int64_t Fout, int exact);

/* Packed W for the forward of K4 / K5 at Fin, Fout <= 64 on a bf16 split: the weight's NS bf16 images (2: bf16x3,
 * 3: bf16x6), cut ONCE per weight version by the arithmetic the kernels use on W itself and stored in the order a wave
 * reads its B fragments,
 *     [column tile j of 16][k-step ks][image s][lane][KF]   bf16,   KF = 8 (4 at Fin = 16), Fin / (4 KF) k-steps,
 *     lane (mi, mh) = (lane & 15, lane >> 4) holding W[16 j + mi][KF (4 ks + mh) .. + KF),
 * so that a kernel loads each fragment as one contiguous run instead of reading fp32 rows of W and splitting them in
 * every wave of every block.  A kernel that reads the images computes bit for bit what it computes from W.
 * gwen_gcn_packw_bytes: size of the images, Fin * Fout * NS * 2; 0 = no packed form (a width outside {16, 32, 64} or a
 *   contract other than GWEN_CONTRACT_BF16X3 / _BF16X6).
 * gwen_gcn_packw_f32: W [Fout, Fin] contiguous -> packed (both 16-byte aligned); one launch on `stream`.  The images
 *   hold for the VALUES W has at that point: pack again after W changes. */
int64_t gwen_gcn_packw_bytes(int64_t Fin, int64_t Fout, int contract);
int gwen_gcn_packw_f32(const float *W, int64_t Fin, int64_t Fout, int contract, void *packed, gwen_stream_t stream);
/* gwen_gcn_layer_tuned2_f32 with the images of W: a fourth choice that CHANGES NO VALUE; gwen_gcn_layer_tuned2_f32
 * forwards with NULL, 0.
 * packed: 1 = W is read and split in the kernel (Wp ignored); 2 = Wp, the gwen_gcn_packw_f32 image of W for (Fin, Fout,
 *   exact), is read and W may be NULL (Fin, Fout <= 64 and exact = GWEN_CONTRACT_BF16X3 / _BF16X6 only; elsewhere, or
 *   with Wp NULL or misaligned, GWEN_EINVAL); 0 = the library's choice: 2 where Wp is given and
 *   gwen_gcn_layer_packed_mode says so, else 1.  packed outside {0, 1, 2}: GWEN_EINVAL.
 * block_rows: the kernels that read images also exist with 80 rows per block at Fin = 64 (five gather passes; four such
 *   blocks of 64 -> 64 on bf16x6 fit a CU's LDS); without images 80 stays GWEN_EINVAL, as in every older entry point. */
int gwen_gcn_layer_tuned3_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *x,
                              const float *W, const float *bias, float *out, int64_t N, int64_t Fin,
                              int64_t Fout, int64_t ldx, int64_t ldo, int64_t members, int64_t mstride_x,
                              int64_t mstride_o, int relu, int exact, int entries, int depth, int block_rows,
                              int index_mode, const void *Wp, int packed, gwen_stream_t stream);
/* For measurements: launches nothing and stores in *blocks_per_cu what hipOccupancyMaxActiveBlocksPerMultiprocessor reports
 * for the kernel the same call of gwen_gcn_layer_tuned3_f32 would launch (asked of the uniform-layout kernel, as the
 * launcher's own co-resident rule does).  Same checks and return codes; N, members > 0. */
int gwen_gcn_layer_blocks_per_cu(const int32_t *rowptr, const int32_t *col, const float *val, const float *x,
                                 const float *W, const float *bias, float *out, int64_t N, int64_t Fin,
                                 int64_t Fout, int64_t ldx, int64_t ldo, int64_t members, int64_t mstride_x,
                                 int64_t mstride_o, int relu, int exact, int entries, int depth, int block_rows,
                                 int index_mode, const void *Wp, int packed, int *blocks_per_cu);
/* what packed = 0 does with an image: 1 = W is split in the kernel, 2 = the image is read (0: unsupported widths / exact) */
int gwen_gcn_layer_packed_mode(int64_t Fin, int64_t Fout, int exact);
/* gwen_gcn_layer_tuned3_f32 with the store mode of the epilogue: a fifth choice that CHANGES NO VALUE;
 * gwen_gcn_layer_tuned3_f32 forwards with 0.
 * store_mode: 1 = plain 16-byte stores of the MFMA result fragments; 3 = the same stores WRITTEN THROUGH (the line goes to
 *   memory at the store and leaves the L2, so the launch leaves no dirty lines behind) -- Fin, Fout <= 64 on
 *   GWEN_CONTRACT_BF16X3 / _BF16X6, uniform layout (rowptr NULL), depth and index_mode 0 or the library's for the shape;
 *   elsewhere GWEN_EINVAL.  2 and 4 (whole rows through LDS, plain and written through) are reserved and not built:
 *   GWEN_EINVAL.  0 = the library's choice (gwen_gcn_layer_store_mode, with one member; 1 otherwise).  Outside 0..4:
 *   GWEN_EINVAL.  All of these are refused before any HIP call. */
int gwen_gcn_layer_tuned4_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *x,
                              const float *W, const float *bias, float *out, int64_t N, int64_t Fin,
                              int64_t Fout, int64_t ldx, int64_t ldo, int64_t members, int64_t mstride_x,
                              int64_t mstride_o, int relu, int exact, int entries, int depth, int block_rows,
                              int index_mode, const void *Wp, int packed, gwen_stream_t stream, int store_mode);
/* what store_mode = 0 runs on a uniform layout with one member: 1 .. 4, and 1 wherever the modes do not exist
 * (0: unsupported widths / exact) */
int gwen_gcn_layer_store_mode(int64_t Fin, int64_t Fout, int exact);
/* gwen_gcn_layer_tuned4_f32 with the row layout of the written-through epilogue: a sixth choice that CHANGES NO VALUE;
 * gwen_gcn_layer_tuned4_f32 forwards with 0 and keeps its store_mode's meaning and refusals (2 and 4 stay reserved).
 * row_stores: 1 = the result tile leaves as the MFMA holds it (16 rows x 64 B per wave instruction); 2 = it leaves as
 *   WHOLE ROWS through an fp32 out tile in LDS (one run of 1024 / (4 Fout) consecutive rows per wave instruction: one
 *   contiguous KiB where ldo == Fout; columns Fout .. ldo - 1 and rows >= N are never written) -- only where store mode 3
 *   is admitted and the resolved store mode is 3; elsewhere GWEN_EINVAL.  0 = the library's choice
 *   (gwen_gcn_layer_row_stores, with one member and a resolved store mode of 3; 1 otherwise).  Outside 0..2: GWEN_EINVAL.
 *   All of these are refused before any HIP call. */
int gwen_gcn_layer_tuned5_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *x,
                              const float *W, const float *bias, float *out, int64_t N, int64_t Fin,
                              int64_t Fout, int64_t ldx, int64_t ldo, int64_t members, int64_t mstride_x,
                              int64_t mstride_o, int relu, int exact, int entries, int depth, int block_rows,
                              int index_mode, const void *Wp, int packed, gwen_stream_t stream, int store_mode,
                              int row_stores);
/* what row_stores = 0 runs on a uniform layout with one member where store_mode = 0 runs mode 3: 1 or 2, and 1 wherever
 * row stores do not exist or the library's store mode is not 3 (0: unsupported widths / exact) */
int gwen_gcn_layer_row_stores(int64_t Fin, int64_t Fout, int exact);

/* ---------------------------------------------------------------------------------------------
 * K8  K4's contract for WIDE layers on locality-ordered bounded-degree graphs (meshes), tile-staged:
 *        out = act( (A~ x) W^T + bias )
 * (the same piece of /root/reference/src/gwen/models_gnn.py:147-149,:204-206 as K4).  Destination rows
 * are cut into tiles of GWEN_TILE_ROWS; per tile the UNION of the source rows its entries name is
 * staged once in LDS by LDS-DMA, 64 features at a time, and the 7-8 gathers per destination row are
 * served from there, overlapped with the 3xbf16 MFMA contraction of the previous chunk.
 *
 * gwen_gcn_tiles64 (part of K1, once per graph; plain CSR in -- rowptr/col/val of gwen_gcn_prep or
 * gwen_gcn_prep_rect, every row at most 8 entries):
 *   t_rows int32 [T * GWEN_TILE_UNION]  the tile's distinct source rows, ascending; a group of 4 slots that
 *                                      starts past the union holds -1, other slots past it the first row
 *   t_lid  u16   [T * 512]             per entry slot (row-in-tile * 8 + k) the rank of its source row in
 *                                      the union; padding slots repeat the row's first entry
 *   t_val  fp32  [T * 512]             per entry slot its weight, 0 for padding slots and rows >= N
 *   status int32 [2]                   status[0] = 1 if some row has more than 8 entries or some tile's
 *                                      union exceeds GWEN_TILE_UNION (K8 must not be used: K4 or K3 + K2
 *                                      instead); status[1] = largest union.  T = gwen_gcn_tiles64_count(N).
 * gwen_gcn_wide_layer_f32: x [members, N_src, Fin] contiguous rows, out [members, N, Fout] row stride ldo;
 *   Fin, Fout in {64, 128, 256} (gwen_gcn_wide_supported); N_src * Fin * 4 < 2^32.  Split contraction `contract`,
 *   fp32 accumulation; the bf16 splits are term for term the arithmetic of gwen_gcn_layer_f32(exact = contract).
 *   union_max = status[1] of gwen_gcn_tiles64 (any upper bound <= GWEN_TILE_UNION is correct): with unions
 *   of at most 128 rows the kernel keeps two chunks of DMA in flight instead of one.
 * ------------------------------------------------------------------------------------------- */
#define GWEN_TILE_ROWS 64
#define GWEN_TILE_UNION 192
int64_t gwen_gcn_tiles64_count(int64_t N);
int gwen_gcn_tiles64(const int32_t *rowptr, const int32_t *col, const float *val, int64_t N,
                     int32_t *t_rows, uint16_t *t_lid, float *t_val, int32_t *status,
                     gwen_stream_t stream);
/* HOST arrays in, HOST array out (no device work): a locality order of the rows of a square prepared CSR whose own
 * numbering has none -- breadth-first balls of GWEN_TILE_ROWS rows grown next to each other over the in-neighbour
 * lists.  perm [N]: new position -> old row.  Relabel the CSR with it (rows permuted, columns mapped through the
 * inverse, entry order inside a row kept) and K8 tiles what it could not before; results stay bitwise those of the
 * unpermuted kernels because every row still sums its entries in stored order. */
int gwen_cluster_rows64_host(const int32_t *rowptr, const int32_t *col, int64_t N, int64_t N_src, int32_t *perm);
int gwen_gcn_wide_supported(int64_t Fin, int64_t Fout);
/* contract: GWEN_CONTRACT_BF16X3 or GWEN_CONTRACT_BF16X6 for every supported width pair (bf16x6 needs tile unions
 * within 128 rows; at 256 -> 256 it runs as two 256 -> 128 launches: three images of W for all 256 output columns
 * exceed the registers of the 8 waves that hold them); GWEN_CONTRACT_F16X3: one launch at every width pair, unions up to
 * GWEN_TILE_UNION rows. */
int gwen_gcn_wide_contract_supported(int64_t Fin, int64_t Fout, int contract);
/* 1 when an AUTO layer of these widths over N rows x members is issued as K8 rather than K4 (given a graph
 * that tiles): every supported width pair with Fin >= 128 (measured 1.15x - 1.6x K4), and Fin = 64 once the
 * layer's input no longer sits in the caches (members * N >= 300 000 rows; equal to K4 below that). */
int gwen_gcn_wide_preferred(int64_t N, int64_t members, int64_t Fin, int64_t Fout);
int gwen_gcn_wide_layer_f32(const int32_t *t_rows, const uint16_t *t_lid, const float *t_val,
                            const float *x, const float *W, const float *bias, float *out, int64_t N,
                            int64_t N_src, int64_t Fin, int64_t Fout, int64_t ldo, int64_t members,
                            int64_t mstride_x, int64_t mstride_o, int relu, int64_t union_max,
                            int contract, gwen_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K5  K4 with the NEXT layer's projection chained on (A~ is linear, so a layer may be gathered at
 * min(Fin, Fout); for a shrinking layer its projection must exist before its gather starts):
 *   pre = 0:  out = act( (A~ x) W1^T + bias ) W2^T     x [.,Fin], W1 [F1,Fin], W2 [F2,F1], F2 < F1
 *   pre = 1:  out = act( A~ h + bias ) W1^T            h [.,Fin] already projected, bias [Fin], F2 = 0
 * rowptr/col/val: GROUPED arrays (rowptr NULL = uniform layout); x, out contiguous rows; widths in {16, 32, 64, 128};
 * contract: GWEN_CONTRACT_BF16X3 or GWEN_CONTRACT_BF16X6, as K4.  The re-bracketing changes fp32 rounding order only.
 * Alignment: x, out, W1, W2 and bias 16-byte aligned; mstride_x and mstride_o (elements) multiples of 4 -- the kernel
 * loads 16-byte vectors at x + m * mstride_x and stores them at out + m * mstride_o -- otherwise GWEN_EINVAL, as K4.
 * ------------------------------------------------------------------------------------------- */
int gwen_gcn_chain_supported(int64_t Fin, int64_t F1, int64_t F2, int pre, int contract);
int gwen_gcn_chain_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *x,
                       const float *W1, const float *W2, const float *bias, float *out, int64_t N,
                       int64_t Fin, int64_t F1, int64_t F2, int pre, int relu, int64_t members,
                       int64_t mstride_x, int64_t mstride_o, int contract, gwen_stream_t stream);
/* entries: as gwen_gcn_layer_entries_f32 (7 acts at Fin, F1 <= 64, the activation-first form included). */
int gwen_gcn_chain_entries_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *x,
                               const float *W1, const float *W2, const float *bias, float *out, int64_t N,
                               int64_t Fin, int64_t F1, int64_t F2, int pre, int relu, int64_t members,
                               int64_t mstride_x, int64_t mstride_o, int contract, int entries, gwen_stream_t stream);
/* depth, block_rows: as gwen_gcn_layer_tuned_f32 -- neither changes a value; gwen_gcn_chain_entries_f32 forwards
 * with 0, 0.  depth 2 acts at Fin, F1 <= 64 (the form without a contraction gathers one pass per wave: both depths
 * are the same code).  block_rows: 0 = the library's choice (64; 128 from Fin = 128 on), or 64 / 96 / 112 at
 * Fin, F1 <= 64 where that is a whole number of gather passes (16 * 64 / Fin rows); the form without a contraction:
 * 0 or its one size, 1024 / Fin.  Otherwise GWEN_EINVAL. */
int gwen_gcn_chain_tuned_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *x,
                             const float *W1, const float *W2, const float *bias, float *out, int64_t N,
                             int64_t Fin, int64_t F1, int64_t F2, int pre, int relu, int64_t members,
                             int64_t mstride_x, int64_t mstride_o, int contract, int entries, int depth,
                             int block_rows, gwen_stream_t stream);
/* the depth gwen_gcn_chain_f32 runs on a uniform layout: 1 or 2 (0: gwen_gcn_chain_supported says no) */
int gwen_gcn_chain_depth(int64_t Fin, int64_t F1, int64_t F2, int pre, int contract);
/* index_mode: as gwen_gcn_layer_tuned2_f32 -- it changes no value; gwen_gcn_chain_tuned_f32 forwards with 0.  Mode 2
 * acts at Fin, F1 <= 64 on the uniform layout (the form without a contraction included); elsewhere GWEN_EINVAL. */
int gwen_gcn_chain_tuned2_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *x,
                              const float *W1, const float *W2, const float *bias, float *out, int64_t N,
                              int64_t Fin, int64_t F1, int64_t F2, int pre, int relu, int64_t members,
                              int64_t mstride_x, int64_t mstride_o, int contract, int entries, int depth,
                              int block_rows, int index_mode, gwen_stream_t stream);
/* the index mode gwen_gcn_chain_f32 runs on a uniform layout: 1 or 2 (0: gwen_gcn_chain_supported says no) */
int gwen_gcn_chain_index_mode(int64_t Fin, int64_t F1, int64_t F2, int pre, int contract);
/* W1p, W2p, packed: as gwen_gcn_layer_tuned3_f32 -- no value changes; gwen_gcn_chain_tuned2_f32 forwards with NULL, NULL,
 * 0.  W1p = gwen_gcn_packw_f32(W1, Fin, F1, contract), W2p = gwen_gcn_packw_f32(W2, F1, F2, contract) (F2 > 0 only).
 * packed = 2 needs Fin, F1 <= 64, a contraction (F1 > 0) and an image for every weight of the form, else GWEN_EINVAL;
 * W1 / W2 may then be NULL.  packed = 0: the images where all are given and gwen_gcn_chain_packed_mode says 2.
 * block_rows: 80 as well at Fin = 64 where the images are read, as K4. */
int gwen_gcn_chain_tuned3_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *x,
                              const float *W1, const float *W2, const float *bias, float *out, int64_t N,
                              int64_t Fin, int64_t F1, int64_t F2, int pre, int relu, int64_t members,
                              int64_t mstride_x, int64_t mstride_o, int contract, int entries, int depth,
                              int block_rows, int index_mode, const void *W1p, const void *W2p, int packed,
                              gwen_stream_t stream);
/* as gwen_gcn_layer_blocks_per_cu, for the kernel gwen_gcn_chain_tuned3_f32 would launch (F1 > 0 only) */
int gwen_gcn_chain_blocks_per_cu(const int32_t *rowptr, const int32_t *col, const float *val, const float *x,
                                 const float *W1, const float *W2, const float *bias, float *out, int64_t N,
                                 int64_t Fin, int64_t F1, int64_t F2, int pre, int relu, int64_t members,
                                 int64_t mstride_x, int64_t mstride_o, int contract, int entries, int depth,
                                 int block_rows, int index_mode, const void *W1p, const void *W2p, int packed,
                                 int *blocks_per_cu);
/* what packed = 0 does with images: 1 or 2 as gwen_gcn_layer_packed_mode (0: gwen_gcn_chain_supported says no) */
int gwen_gcn_chain_packed_mode(int64_t Fin, int64_t F1, int64_t F2, int pre, int contract);
/* store_mode: as gwen_gcn_layer_tuned4_f32 -- no value changes; gwen_gcn_chain_tuned3_f32 forwards with 0.  3 needs Fin,
 * F1 <= 64 (F1 = 0, the plain gather, included), the uniform layout, and depth and index_mode 0 or the library's. */
int gwen_gcn_chain_tuned4_f32(const int32_t *rowptr, const int32_t *col, const float *val, const float *x,
                              const float *W1, const float *W2, const float *bias, float *out, int64_t N,
                              int64_t Fin, int64_t F1, int64_t F2, int pre, int relu, int64_t members,
                              int64_t mstride_x, int64_t mstride_o, int contract, int entries, int depth,
                              int block_rows, int index_mode, const void *W1p, const void *W2p, int packed,
                              gwen_stream_t stream, int store_mode);
/* what store_mode = 0 runs on a uniform layout with one member: 1 .. 4 (0: gwen_gcn_chain_supported says no) */
int gwen_gcn_chain_store_mode(int64_t Fin, int64_t F1, int64_t F2, int pre, int contract);

/* ---------------------------------------------------------------------------------------------
 * Whole-stack forward == GNNModel.forward (/root/reference/src/gwen/models_gnn.py:292-303 ->
 * :241-258 -> :135-157, :189-212): every layer of the stack issued back to back from one host
 * call, so the host never limits the device (the reference pays ~15 eager launches per layer).
 *
 * layers (HOST array): per layer W [fout, fin], bias [fout] or NULL (device pointers), relu 0/1 and
 *   order: GWEN_ORDER_AUTO picks K4 when gwen_gcn_layer_supported(fin, fout) -- and chains the next
 *   layer's projection (K5) when that layer is AUTO too and shrinks, so that it is gathered at its
 *   narrow width -- otherwise transform-first (K3 then K2) when fout <= fin, aggregate-first (K2
 *   then K3) when fin < fout.  Explicit orders are taken literally, layer by layer.
 * graph (HOST struct of device pointers): rowptr/col/val = the prepared CSR (K2 layers); g_rowptr/g_col/g_val
 *   = its grouped form (K4/K5 layers; g_col/g_val may be NULL when no layer resolves to K4/K5, g_rowptr
 *   NULL = uniform layout); dense = the graph as a dense padded matrix (gwen_gcn_dense_f32) or NULL -- when
 *   given and every layer is AUTO and gwen_gcn_small_supported(N, fin, fout), every layer is ONE K7 launch;
 *   t_rows/t_lid/t_val/union_max = the tile layout of gwen_gcn_tiles64 or NULL -- when given, AUTO layers
 *   with gwen_gcn_wide_preferred() run as K8.
 * x [members, N, layers[0].fin] and out [members, N, layers[n-1].fout] contiguous; out != x.
 * scratch: fp32 workspace of gwen_gnn_forward_scratch_floats() elements (16-byte aligned).
 * acts (HOST array of n_layers device pointers, or NULL): the TRAINING forward -- layer l's output is
 *   stored in acts[l] ([members, N, layers[l].fout]; acts[n_layers-1] may be `out`) and no projection is
 *   chained across layers (every activation the backward needs exists).
 * events (HOST array of hipEvent_t, or NULL): if given, events[2i] / events[2i+1] are recorded on
 *   `stream` right before / after kernel launch i; info[i] (HOST, or NULL) says what launch i was.
 *   n_launches (HOST, or NULL) receives the number of launches; max_launches bounds both arrays.
 * ------------------------------------------------------------------------------------------- */
#define GWEN_ORDER_AUTO (-1)
#define GWEN_ORDER_TRANSFORM_FIRST 0
#define GWEN_ORDER_AGGREGATE_FIRST 1
#define GWEN_ORDER_FUSED 2         /* K4, split contraction (gwen_layer_desc.contract) */
#define GWEN_ORDER_FUSED_EXACT 3   /* K4, fp32 MFMA contraction */
#define GWEN_KIND_LINEAR 3      /* K3 */
#define GWEN_KIND_PROPAGATE 2   /* K2 */
#define GWEN_KIND_LAYER 4       /* K4 */
#define GWEN_KIND_CHAIN 5       /* K5: info.fin = gathered width, info.fout = stored width */
#define GWEN_KIND_SMALL 6       /* K7: whole layer on a small graph (dense adjacency) */
#define GWEN_KIND_WIDE 8        /* K8: whole layer, tile-staged */

typedef struct gwen_graph {
  int64_t N;                          /* nodes (rows of x and out) */
  const int32_t *rowptr, *col;        /* gwen_gcn_prep */
  const float *val;
  const int32_t *g_rowptr, *g_col;    /* gwen_gcn_group8 (g_rowptr NULL = uniform) or NULL */
  const float *g_val;
  const float *dense;                 /* gwen_gcn_dense_f32 or NULL */
  const int32_t *t_rows;              /* gwen_gcn_tiles64 or NULL */
  const uint16_t *t_lid;
  const float *t_val;
  int64_t union_max;
} gwen_graph;

typedef struct gwen_layer_desc {
  const float *W;
  const float *bias;
  int32_t fin, fout, relu, order;
  const void *packed;  /* gwen_gcn_small_pack_f32 image of W for K7, or NULL */
  int32_t contract;    /* AUTO / FUSED layers: GWEN_CONTRACT_BF16X3, _BF16X6 or _F16X3 (fp32-class on the kernel's own
                          split, see above); explicit transform-first / aggregate-first / FUSED_EXACT orders
                          contract in fp32 */
  int32_t reserved;
} gwen_layer_desc;

typedef struct gwen_launch_info {
  int32_t kind, layer, fin, fout;
} gwen_launch_info;

int64_t gwen_gnn_forward_scratch_floats(int64_t N, int64_t members, const gwen_layer_desc *layers,
                                        int32_t n_layers);
int gwen_gnn_forward_f32(const gwen_graph *graph, const gwen_layer_desc *layers, int32_t n_layers,
                         const float *x, float *out, float *scratch, int64_t scratch_floats,
                         int64_t members, gwen_stream_t stream, void **events,
                         gwen_launch_info *info, int32_t max_launches, int32_t *n_launches,
                         float *const *acts);
/* entries: handed to every K4 / K5 launch of the stack (gwen_gcn_layer_entries_f32); 8 = gwen_gnn_forward_f32. */
int gwen_gnn_forward_entries_f32(const gwen_graph *graph, const gwen_layer_desc *layers, int32_t n_layers,
                                 const float *x, float *out, float *scratch, int64_t scratch_floats,
                                 int64_t members, gwen_stream_t stream, void **events,
                                 gwen_launch_info *info, int32_t max_launches, int32_t *n_launches,
                                 float *const *acts, int entries);
/* The same, handed the packed images of the layers' weights for the K4 / K5 launches of the stack.
 * packw (HOST array of n_layers device pointers, or NULL; any element may be NULL): packw[l] =
 *   gwen_gcn_packw_f32(layers[l].W, fin, fout, c) with c the layer's contraction in K4 / K5 (GWEN_CONTRACT_F16X3 layers:
 *   _BF16X6).  A launch reads images only when it has one for every weight it contracts with.
 * packed: 0 = each launch's own choice (gwen_gcn_layer_packed_mode / gwen_gcn_chain_packed_mode), 1 = never,
 *   2 = wherever the images are given.  No value changes.  The training forward (acts) reads no images.
 * gwen_gnn_forward_entries_f32 forwards with NULL, 0. */
int gwen_gnn_forward_packed_f32(const gwen_graph *graph, const gwen_layer_desc *layers, int32_t n_layers,
                                const float *x, float *out, float *scratch, int64_t scratch_floats,
                                int64_t members, gwen_stream_t stream, void **events,
                                gwen_launch_info *info, int32_t max_launches, int32_t *n_launches,
                                float *const *acts, int entries, const void *const *packw, int packed);

/* ---------------------------------------------------------------------------------------------
 * K7  a whole GCNConv layer on a SMALL graph (N <= 256) with wide features -- the reference's own
 * shape: the complete graph over ~125-150 ensemble members (/root/reference/src/gwen/utils.py:175-176),
 * features = flattened fields, hidden 1024 (/root/reference/src/gwen/config.json:9,12).
 *   gwen_gcn_dense_f32: dense[i*NP + j] = sum of the stored weights of entries (i <- j) of a prepared
 *     square CSR (K1), zero elsewhere; NP = gwen_gcn_small_pad(N) = 128 or 256; dense: fp32 [NP*NP].
 *   gwen_gcn_small_layer_f32: out[m] = act( dense (x[m] W^T) + bias ), x [members, N, Fin] contiguous
 *     rows (member stride mstride_x), W [Fout, Fin], out [members, N, Fout]; Fin % 32 == 0,
 *     Fout % 16 == 0 (gwen_gcn_small_supported).  Both contractions on the bf16 split `contract` names
 *     (GWEN_CONTRACT_BF16X3 or _BF16X6; the packed images serve bf16x3 only: with bf16x6 W is read and split
 *     in the kernel), fp32 accumulation; the aggregation is a dense contraction, so only the summation order
 *     differs from K2's.
 *     workspace: gwen_gcn_small_workspace_floats() fp32 elements (0 unless K is cut over blocks).
 *   gwen_gcn_small_pack_f32: W -> its 3xbf16 hi / lo images in MFMA fragment order
 *     (gwen_gcn_small_pack_bytes() bytes, as many as W itself); pass the result as `packed` (W may then
 *     be NULL) and the kernel streams the weights as one contiguous run per column tile -- worth it
 *     when the weights are reused (inference): the C -> 1024 and 1024 -> C layers are bound by reading W.
 * ------------------------------------------------------------------------------------------- */
int gwen_gcn_small_pad(int64_t N);
int gwen_gcn_small_supported(int64_t N, int64_t Fin, int64_t Fout, int contract);
int64_t gwen_gcn_small_workspace_floats(int64_t N, int64_t members, int64_t Fin, int64_t Fout);
int gwen_gcn_dense_f32(const int32_t *rowptr, const int32_t *col, const float *val, int64_t N,
                       float *dense, gwen_stream_t stream);
int64_t gwen_gcn_small_pack_bytes(int64_t Fin, int64_t Fout);
int gwen_gcn_small_pack_f32(const float *W, int64_t Fin, int64_t Fout, void *packed,
                            gwen_stream_t stream);
int gwen_gcn_small_layer_f32(const float *dense, const float *x, const float *W, const void *packed,
                             const float *bias, float *out, int64_t N, int64_t Fin, int64_t Fout,
                             int64_t members,
                             int64_t mstride_x, int64_t mstride_o, int relu, float *workspace,
                             int64_t workspace_floats, int contract, gwen_stream_t stream);

/* hipEvent plumbing for callers without a HIP binding (bench.py times kernels with these, on the
 * stream the kernels are launched on). */
int gwen_event_create(void **event /* host out */);
int gwen_event_destroy(void *event);
int gwen_event_record(void *event, gwen_stream_t stream);
int gwen_event_synchronize(void *event);
int gwen_event_elapsed_ms(void *start, void *stop, float *ms /* host out */);

/* ---------------------------------------------------------------------------------------------
 * Backward pieces (autograd of the layer; the reference trains through it:
 * /root/reference/src/gwen/models_gnn.py:372 loss.backward()).
 *   grad_W[Fout,Fin] = g^T @ x   (g [rows,Fout], x [rows,Fin]); deterministic two-stage reduce.  contract: the
 *                      contraction of the layer the gradient belongs to -- GWEN_CONTRACT_F32: fp32-input MFMA (exact
 *                      fp32 products); _BF16X3 / _BF16X6 (_F16X3 = _BF16X6 here): the split contractions on 64 x 64
 *                      tiles of grad_W, operands staged through LDS, where Fin and Fout are multiples of 64 (at 256
 *                      channels 2.7 - 3.7 x the fp32 MFMA's rate), the fp32 MFMA elsewhere.
 *   grad_b[F]        = column sums of g.
 *   relu mask        : g *= (y > 0).
 * partial: fp32 workspace of gwen_gcn_grad_workspace_floats(rows, Fin, Fout) elements.
 * ------------------------------------------------------------------------------------------- */
int64_t gwen_gcn_grad_workspace_floats(int64_t rows, int64_t Fin, int64_t Fout);
int gwen_gcn_grad_weight_f32(const float *g, const float *x, float *grad_W, int64_t rows,
                             int64_t Fin, int64_t Fout, int64_t ldg, int64_t ldx, float *partial,
                             int contract, gwen_stream_t stream);
int gwen_gcn_grad_bias_f32(const float *g, float *grad_b, int64_t rows, int64_t F, int64_t ldg,
                           float *partial, gwen_stream_t stream);
int gwen_relu_backward_f32(const float *y, const float *g, float *gin, int64_t count,
                           gwen_stream_t stream);
/* Building blocks of gwen_gnn_backward_f32: stage 1 of the two reductions alone (per-chunk partial sums,
 * [gwen_gcn_grad_weight_chunks(rows, Fin, Fout, contract) <= gwen_gcn_grad_chunks(rows), Fout * Fin] and
 * [gwen_gcn_grad_chunks(rows), F]), the fixed-order finish of up to
 * GWEN_MAX_REDUCE_TASKS such reductions in ONE launch (dst[j] = sum over chunks of partial[c * count + j]),
 * and up to GWEN_MAX_REDUCE_TASKS small transposes (wt [cols, rows] = w [rows, cols]^T) in one launch.
 * tasks / w / wt / rows / cols are HOST arrays (they travel as kernel arguments). */
#define GWEN_MAX_REDUCE_TASKS 32
typedef struct gwen_reduce_task {
  const float *partial;
  float *dst;
  int64_t count, nchunks;
} gwen_reduce_task;
int64_t gwen_gcn_grad_chunks(int64_t rows);
int64_t gwen_gcn_grad_weight_chunks(int64_t rows, int64_t Fin, int64_t Fout, int contract);
int gwen_gcn_grad_weight_partial_f32(const float *g, const float *x, float *partial, int64_t rows,
                                     int64_t Fin, int64_t Fout, int64_t ldg, int64_t ldx, int contract,
                                     gwen_stream_t stream);
int gwen_gcn_grad_bias_partial_f32(const float *g, float *partial, int64_t rows, int64_t F, int64_t ldg,
                                   gwen_stream_t stream);
/* Stage 1 of grad_W = g^T x AND of grad_b = column sums of g in ONE launch (the g tile is staged anyway), where the
 * weight gradient runs on the LDS-staged split kernel: gwen_gcn_grad_weight_bias_supported(Fin, Fout, contract) -- widths
 * that are multiples of 64 on a split contraction; g, x 16-byte aligned with ldg, ldx multiples of 4 (GWEN_EINVAL
 * otherwise: use the two separate launches).  partial_w as above; partial_b [gwen_gcn_grad_weight_chunks(...), Fout]. */
int gwen_gcn_grad_weight_bias_supported(int64_t Fin, int64_t Fout, int contract);
int gwen_gcn_grad_weight_bias_partial_f32(const float *g, const float *x, float *partial_w, float *partial_b,
                                          int64_t rows, int64_t Fin, int64_t Fout, int64_t ldg, int64_t ldx,
                                          int contract, gwen_stream_t stream);
int gwen_reduce_chunks_batched(const gwen_reduce_task *tasks, int32_t n_tasks, gwen_stream_t stream);
int gwen_transpose_batched(const float *const *w, float *const *wt, const int32_t *rows,
                           const int32_t *cols, int32_t n, gwen_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Backward of a whole layer / of the whole stack (the reference's loss.backward(),
 * /root/reference/src/gwen/models_gnn.py:372, through six GCNConv layers).
 *
 * gwen_gcn_layer_bwd_f32: K4's kernel on the TRANSPOSED graph (t_* = gwen_gcn_group8 of gwen_gcn_transpose):
 *     gh = A~^T g                         stored (the operand of grad_W = gh^T x); gh may be NULL
 *     gx = (gh Wt^T) masked by mask > 0   Wt [Fx, Fg] = the layer's lin.weight ([Fg, Fx]) transposed;
 *                                         mask = the output of the layer below when it has a ReLU, or NULL
 *   g, gh [members, N, Fg]; gx, mask [members, N, Fx], contiguous; widths as gwen_gcn_layer_supported(Fg, Fx);
 *   contract: GWEN_CONTRACT_BF16X3 or GWEN_CONTRACT_BF16X6 -- the split of the gx contraction.
 * gwen_gnn_backward_f32: all layers, last to first, from one host call: per layer grad_b (column sums of
 *   the incoming, already masked gradient), the launch above (or K2^T + K3 + mask where the widths are not
 *   K4's) on the LAYER'S OWN precision (bf16x3 layers: bf16x3; bf16x6 / f16x3 layers: bf16x6; explicit fp32
 *   orders: the fp32-input MFMA), grad_W (fp32-input MFMA reductions).  graph_t: the views of the TRANSPOSED graph (rowptr/col/val and, for the fused launch,
 *   g_rowptr/g_col/g_val).  acts (HOST array of n_layers device pointers): every layer's output as the
 *   training forward stored it (gwen_gnn_forward_f32 with acts); x: the stack's input; grad_out: gradient of
 *   the last layer's output.  grad_x may be NULL; grad_W / grad_b: HOST arrays of device pointers (NULL array
 *   or NULL entry = not wanted).  scratch: gwen_gnn_backward_scratch_floats() fp32 elements.
 * ------------------------------------------------------------------------------------------- */
int gwen_gcn_layer_bwd_f32(const int32_t *t_rowptr, const int32_t *t_col, const float *t_val,
                           const float *g, const float *Wt, const float *mask, float *gh, float *gx,
                           int64_t N, int64_t Fg, int64_t Fx, int64_t members, int contract, gwen_stream_t stream);
/* The same launch with stage 1 of the grad_b of the layer BELOW as well: gx is that layer's incoming gradient, and its
 * column sums per (member, chunk of rows) cost the kernel one LDS turn -- *bias_chunks (a HOST integer, written by
 * this call) partial rows of Fx floats go to bias_partial (room for gwen_gcn_layer_bwd_bias_rows(N, members) rows),
 * every one written exactly once; gwen_reduce_chunks_batched finishes them in a fixed order.  bias_partial and
 * bias_chunks both NULL: gwen_gcn_layer_bwd_f32. */
int64_t gwen_gcn_layer_bwd_bias_rows(int64_t N, int64_t members);
int gwen_gcn_layer_bwd_bias_f32(const int32_t *t_rowptr, const int32_t *t_col, const float *t_val, const float *g,
                                const float *Wt, const float *mask, float *gh, float *gx, int64_t N, int64_t Fg,
                                int64_t Fx, int64_t members, int contract, float *bias_partial,
                                int64_t *bias_chunks, gwen_stream_t stream);
int64_t gwen_gnn_backward_scratch_floats(int64_t N, int64_t members, const struct gwen_layer_desc *layers,
                                         int32_t n_layers);
int gwen_gnn_backward_f32(const struct gwen_graph *graph_t, const struct gwen_layer_desc *layers,
                          int32_t n_layers, const float *x, const float *const *acts,
                          const float *grad_out, float *grad_x, float *const *grad_W,
                          float *const *grad_b, float *scratch, int64_t scratch_floats, int64_t members,
                          gwen_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K6 -- InteractionNet block: edge MLP + sum to target nodes, and the node MLP  (SURVEY 8(f) f2).
 * BUILD-DEFINED: the reference has no edge MLP (its layers are the GCNConv calls at
 * /root/reference/src/gwen/models_gnn.py:147-149,:204-206); BASELINE.json's north_star names the
 * block, semantics follow the published Interaction Network formulation restated in
 * oracle/interaction_oracle.py (PARITY UNPINNED).
 *
 * gwen_mlp2_f32, for rows r = 0 .. R-1 of width F (gwen_mlp2_supported):
 *     pre[r] = A[r] W1^T + G1[idx1 ? idx1[r] : r] + G2[idx2 ? idx2[r] : r] + b1    (G1, G2 optional)
 *     y[r]   = act(pre[r]) W2^T + b2                       act: GWEN_ACT_NONE / RELU / SILU
 *     out[r] = res[r] + y[r]                               (out, res optional; out may alias A / res)
 *     agg[d] = sum (or mean) of y[r] over rows r with rowptr[d] <= r < rowptr[d+1]   (agg optional)
 *   A, G*, res, out: fp32 row-major, contiguous rows of F; W1, W2: [F,F] row-major [out,in].
 *   G1 / G2 have G1_rows / G2_rows rows with row stride ldg1 / ldg2 floats (>= F, multiple of 4;
 *   rows * ld * 4 < 2^32 -- a table may be a column block of a wider matrix, e.g. one of several
 *   projections computed by a single K3 launch); supported table pairs: none; G1 alone
 *   (with or without idx1); G1 and G2 both indexed.  GWEN_EINVAL otherwise.
 *   With agg: rows are the stored entries of a target-sorted CSR (rowptr int32 [N_agg+1],
 *   rowptr[N_agg] == R) and tile_row [n_tiles+1] comes from gwen_edge_tiles; every target row is
 *   summed by one block in stored order (no atomics; rows without entries get 0).
 *   The contractions use the 3xbf16 split (see gwen_gcn_layer_f32, exact = 0).
 *   workspace: gwen_mlp2_workspace_bytes(F) bytes, 16-byte aligned (GWEN_ENOSPACE if smaller): only F = 256
 *   needs one -- its weights are streamed from pre-split bf16 fragment images (F = 64 splits them in-kernel).
 *
 * gwen_mlp2_contract_f32 / gwen_mlp2_bwd_contract_f32: the same launches with a choice of contraction (contract, a
 *   GWEN_CONTRACT_* code; gwen_mlp2_contract_supported(F, contract)): GWEN_CONTRACT_BF16X3 is gwen_mlp2_f32 /
 *   gwen_mlp2_bwd_f32 bit for bit (they forward to it); GWEN_CONTRACT_F16X3 is "fp32-class on the kernel's own split",
 *   as on gwen_layer_desc: two fp16 images per operand at the same three MFMAs per k-step, both operands scaled by
 *   exact powers of two -- W per OUTPUT COLUMN, the A rows and the activated hidden rows per ROW (a row's result never
 *   depends on the other rows of a launch: a member of a block-diagonal batched launch is bitwise the member alone).
 *   Each contraction accumulates from zero and is un-scaled by ONE ldexp per element (the two exponents summed) before
 *   G1 / G2 / b1 / b2 / res are added, so an addend far larger or smaller than A W1^T puts no intermediate out of
 *   range.  Accuracy: ~2^-24 relative per product, like bf16x6; elements more than 2^17 below their row's (or W
 *   column's) maximum fall into fp16's subnormal range and keep an ABSOLUTE accuracy of ~2^-40 of that maximum, and
 *   maxima below 2^-107 are scaled as 2^-107 (rows of magnitude 2^-107 .. 2^127 keep full precision; an all-zero
 *   row contributes an exact 0 to A W1^T).  A row holding +-Inf or NaN gets NaN / Inf in every column of that row's outputs (the lo
 *   image of an infinite value is Inf - Inf) and, with agg, in its target's sum; every other row is untouched.  A
 *   non-finite W entry spoils its output column for every row, as in fp32.  Supported: BF16X3 and F16X3 at every F
 *   of gwen_mlp2_supported (the backward: F in {64, 256}); GWEN_CONTRACT_F32 / BF16X6 return GWEN_EINVAL.
 *   workspace: gwen_mlp2_contract_workspace_bytes(F, contract) (F = 256: the images + 2 F int32 column exponents).
 *
 * gwen_mlp2_ln_f32: gwen_mlp2_contract_f32 with a LayerNorm behind the second layer, before the residual and the sums:
 *     y[r] = LN(act(pre[r]) W2^T + b2),   LN(m)_c = (m_c - mu) * rstd * ln_gamma_c + ln_beta_c,
 *     mu = mean_c m_c,  var = mean_c (m_c - mu)^2 (BIASED),  rstd = 1 / sqrt(var + ln_eps)      (torch.nn.LayerNorm(F))
 *   ln_gamma, ln_beta: fp32 [F], 16-byte aligned; both NULL: gwen_mlp2_contract_f32, the same launch bit for bit; one
 *   NULL: GWEN_EINVAL.  ln_eps >= 0 (1e-5 is the usual value).  Statistics and the affine step are fp32 on both
 *   contracts (the contract governs the two contractions only); the variance is formed from DEVIATIONS about the mean
 *   in a second sweep over the row, never as E[m^2] - mu^2 (which loses rows whose mean is large against their
 *   spread).  A row holding +-Inf or NaN gets NaN in every column of y (its mean is non-finite) and, with agg, in its
 *   target's sum; every other row is untouched.  Fused instantiations exist for the launch shapes of the
 *   InteractionNet block only -- gwen_mlp2_ln_supported(F, contract, shape): GWEN_MLP2_LN_EDGE = G1 and G2 both
 *   indexed, agg, res == A (out optional); GWEN_MLP2_LN_NODE = G1 row for row, no G2, no agg, res != A -- at F = 64
 *   (F = 256: the instantiations spill and are not built); every other call with ln_gamma returns GWEN_EINVAL before any launch, and the caller runs
 *   gwen_mlp2_contract_f32 without res / agg followed by ONE gwen_layer_norm_f32 (same semantics).
 *
 * gwen_edge_tiles: row-aligned tiling of a CSR's entries.  tile c owns the target rows whose first
 *   entry lies in [cT, (c+1)T); n_tiles = gwen_edge_tiles_count(E, T) = max(1, ceil(E/T)); T <= 128.
 *   T = gwen_mlp2_rows(F) - (max row length - 1) (at least 1) keeps each tile a single pass of the
 *   kernel at width F; any T is correct (longer tiles take several passes).
 *   Also writes dst[e] = target row of entry e (int32 [E]) -- idx2 of the edge MLP.
 * ------------------------------------------------------------------------------------------- */
#define GWEN_ACT_NONE 0
#define GWEN_ACT_RELU 1
#define GWEN_ACT_SILU 2
int gwen_mlp2_supported(int64_t F);          /* F in {32, 64, 128, 256} */
int gwen_mlp2_rows(int64_t F);                /* rows one pass of the kernel takes at width F (128 at F = 64 and 256, else 64) */
int64_t gwen_mlp2_workspace_bytes(int64_t F); /* F = 256: room for the pre-split weight images; else 0 */
int64_t gwen_edge_tiles_count(int64_t E, int64_t T);
int gwen_edge_tiles(const int32_t *rowptr, int64_t N, int64_t E, int64_t T, int32_t *tile_row,
                    int32_t *dst, gwen_stream_t stream);
int gwen_mlp2_f32(const float *A, const float *W1, const float *G1, const int32_t *idx1,
                  int64_t G1_rows, int64_t ldg1, const float *G2, const int32_t *idx2,
                  int64_t G2_rows, int64_t ldg2,
                  const float *b1, const float *W2, const float *b2, const float *res, float *out,
                  int64_t R, int64_t F, int act, const int32_t *rowptr, const int32_t *tile_row,
                  int64_t n_tiles, float *agg, int64_t N_agg, int mean, void *workspace,
                  size_t workspace_bytes, gwen_stream_t stream);
int gwen_mlp2_contract_supported(int64_t F, int contract);   /* BF16X3 and F16X3 at F in {32, 64, 128, 256} */
int64_t gwen_mlp2_contract_workspace_bytes(int64_t F, int contract);
int gwen_mlp2_contract_f32(const float *A, const float *W1, const float *G1, const int32_t *idx1,
                           int64_t G1_rows, int64_t ldg1, const float *G2, const int32_t *idx2,
                           int64_t G2_rows, int64_t ldg2,
                           const float *b1, const float *W2, const float *b2, const float *res, float *out,
                           int64_t R, int64_t F, int act, const int32_t *rowptr, const int32_t *tile_row,
                           int64_t n_tiles, float *agg, int64_t N_agg, int mean, int contract, void *workspace,
                           size_t workspace_bytes, gwen_stream_t stream);
#define GWEN_MLP2_LN_EDGE 0
#define GWEN_MLP2_LN_NODE 1
int gwen_mlp2_ln_supported(int64_t F, int contract, int shape);
int gwen_mlp2_ln_f32(const float *A, const float *W1, const float *G1, const int32_t *idx1,
                     int64_t G1_rows, int64_t ldg1, const float *G2, const int32_t *idx2,
                     int64_t G2_rows, int64_t ldg2,
                     const float *b1, const float *W2, const float *b2, const float *res, float *out,
                     int64_t R, int64_t F, int act, const int32_t *rowptr, const int32_t *tile_row,
                     int64_t n_tiles, float *agg, int64_t N_agg, int mean, int contract,
                     const float *ln_gamma, const float *ln_beta, float ln_eps, void *workspace,
                     size_t workspace_bytes, gwen_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Row LayerNorm, forward and backward (csrc/layernorm.hip) -- the unfused route of K6 with LayerNorm, the LayerNorm
 * half of the InteractionNet block's backward, and gwen_amd.ops.layer_norm.  BUILD-DEFINED like the block; LN, eps,
 * the biased variance and the deviations form exactly as under gwen_mlp2_ln_f32.  x, res, out, g, gx: fp32
 * [rows, F] contiguous; gamma, beta: [F]; everything 16-byte aligned; gwen_layer_norm_supported(F): F % 4 == 0,
 * F <= 1024.  A row holding +-Inf or NaN gets NaN in every column (and in its target's agg row / in its chunk of the
 * gamma / beta partials); other rows are untouched.
 *   gwen_layer_norm_f32:      out[r] = (res ? res[r] : 0) + LN(x[r])     (out may alias x or res row for row).
 *                             With agg (then rowptr int32 [N_agg + 1], rowptr[N_agg] == rows: rows stored by target):
 *                             agg[d] = sum (mean != 0: mean) of LN(x[r]) over rowptr[d] <= r < rowptr[d + 1], in stored
 *                             order -- of LN(x), not of out; targets without rows get 0; out may then be NULL.
 *   gwen_layer_norm_bwd_f32:  with y^ = (x - mu) rstd recomputed and gg = g * gamma:
 *                             gx[r] = rstd (gg - mean_c(gg) - y^ mean_c(gg * y^))      (gx may alias g, not x);
 *                             partial (may be NULL) [gwen_layer_norm_bwd_chunks(rows), 2 F]: per chunk of 256 rows
 *                             [sum_r g * y^ | sum_r g] in a fixed order; grad_gamma | grad_beta = the sum over chunks
 *                             (gwen_reduce_chunks_batched with count = 2 F).  Atomic-free: two runs bitwise equal.
 * ------------------------------------------------------------------------------------------- */
int gwen_layer_norm_supported(int64_t F);
int gwen_layer_norm_f32(const float *x, const float *gamma, const float *beta, float eps, const float *res, float *out,
                        int64_t rows, int64_t F, const int32_t *rowptr, float *agg, int64_t N_agg, int mean,
                        gwen_stream_t stream);
int64_t gwen_layer_norm_bwd_chunks(int64_t rows);
int gwen_layer_norm_bwd_f32(const float *x, const float *g, const float *gamma, float eps, float *gx, float *partial,
                            int64_t rows, int64_t F, gwen_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K6^T  pieces of the InteractionNet block's BACKWARD (build-defined like K6; serves the training step of the
 * reference's loop shape, /root/reference/src/gwen/models_gnn.py:372-373, for the InteractionNet forecaster).
 * The host (gwen_amd/interaction.py) assembles the backward from K3 (dense products), K2 over CSRs whose columns
 * are edge positions (sums over the edges of a target / source, in stored order), the weight / bias gradient
 * reductions below K4's backward, and these three: every launch is atomic-free with a fixed summation order.
 *   gwen_act_pair_f32:   pre[r] = a[r] + g1[idx1 ? idx1[r] : r] + g2[idx2 ? idx2[r] : r]  (tables optional, row
 *                        strides ld1 / ld2 >= F);  h[r] = act(pre[r]);  dact[r] = act'(pre[r])  (dact may be NULL;
 *                        h may alias a).  a, h, dact: [rows, F] contiguous, F % 4 == 0.
 *   gwen_act_pair_seg_f32: the same for edges STORED BY TARGET (rows rowptr[d] .. rowptr[d + 1] belong to target d, g2 is
 *                        the target's own row: g2[d]) with the per-target sums of h in stored order as well,
 *                        hsum[d] = sum_r h[r]  [n_dst, F] -- gwen_act_pair_f32 followed by K2 over the edge-position
 *                        CSR, bit for bit, without the second pass over [rows, F].
 *   gwen_gather_add_f32: out[r] = (a ? a[r] : 0) + t[idx[r]] * (scale ? scale[idx[r]] : 1)   t: [*, F] contiguous.
 *   gwen_ew_f32:         out = a * b (GWEN_EW_MUL) or a + b (GWEN_EW_ADD), n % 4 == 0; out may alias a or b.
 *   gwen_mlp2_bwd_f32 (round 4): the edge-level half of the backward as ONE launch of K6's row-stationary kernel, at
 *                        64 and 256 channels (gwen_mlp2_bwd_supported):
 *                            g_pre1[r] = (ge[r] W2 + T[dst[r]]) * d1[r]        g_e[r] = ge[r] + g_pre1[r] We
 *                        with T = (g_agg, scaled by 1 / degree for the mean) W2 computed per NODE, so that the message
 *                        gradient ge + g_agg[dst] is never formed; W2t = W2^T, Wet = We^T ([F, F] row-major: row =
 *                        output column); d1 = act'(pre1) [R, F]; T [T_rows, F] with row stride ldT.  g_pre1 has
 *                        gwen_mlp2_bwd_rows(R) rows (R rounded up to whole passes: the kernel stores every lane), g_e
 *                        [R, F] may be ge itself.  workspace as gwen_mlp2_f32.  3xbf16 contractions, as K6.
 *   gwen_mlp2_bwd_contract_f32: the same with a contract (BF16X3 = gwen_mlp2_bwd_f32 bit for bit; F16X3 as
 *                        gwen_mlp2_contract_f32 -- T[dst] is added after the first contraction is un-scaled);
 *                        workspace: gwen_mlp2_contract_workspace_bytes(F, contract).
 * ------------------------------------------------------------------------------------------- */
#define GWEN_EW_MUL 0
#define GWEN_EW_ADD 1
int gwen_act_pair_f32(const float *a, const float *g1, const int32_t *idx1, int64_t ld1, const float *g2,
                      const int32_t *idx2, int64_t ld2, float *h, float *dact, int64_t rows, int64_t F, int act,
                      gwen_stream_t stream);
int gwen_act_pair_seg_f32(const float *a, const float *g1, const int32_t *idx1, int64_t ld1, const float *g2,
                          int64_t ld2, const int32_t *rowptr, float *h, float *dact, float *hsum, int64_t rows,
                          int64_t n_dst, int64_t F, int act, gwen_stream_t stream);
int gwen_gather_add_f32(const float *a, const float *t, const int32_t *idx, const float *scale, float *out,
                        int64_t rows, int64_t F, gwen_stream_t stream);
int gwen_ew_f32(int op, const float *a, const float *b, float *out, int64_t n, gwen_stream_t stream);
int gwen_mlp2_bwd_supported(int64_t F);
int64_t gwen_mlp2_bwd_rows(int64_t R);
int gwen_mlp2_bwd_f32(const float *ge, const float *W2t, const float *d1, const float *T, const int32_t *dst,
                      int64_t T_rows, int64_t ldT, const float *Wet, float *g_pre1, float *g_e, int64_t R, int64_t F,
                      void *workspace, size_t workspace_bytes, gwen_stream_t stream);
int gwen_mlp2_bwd_contract_f32(const float *ge, const float *W2t, const float *d1, const float *T, const int32_t *dst,
                               int64_t T_rows, int64_t ldT, const float *Wet, float *g_pre1, float *g_e, int64_t R,
                               int64_t F, int contract, void *workspace, size_t workspace_bytes, gwen_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Masked L1 loss, value and gradient in one pass -- the reference's training objective
 * (/root/reference/src/gwen/models_gnn.py:261-265: F.l1_loss(output[mask], target[mask]); backward :372):
 *     loss[0] = sum_{m, r : mask[r], c} |out[m,r,c] - target[m,r,c]| / (picked * C * members)
 *     grad[m,r,c] = sign(out - target) * mask[r] / (picked * C * members)      (grad may be NULL)
 * out, target, grad: fp32 [members, N, C] contiguous, C % 4 == 0, 16-byte aligned; mask: one byte per row [N]
 * (non-zero = selected); picked = number of selected rows (0 => NaN, as torch).  Three launches, sums in a
 * fixed order (bitwise reproducible).  workspace: gwen_masked_l1_workspace_floats() floats.
 * ------------------------------------------------------------------------------------------- */
int64_t gwen_masked_l1_workspace_floats(void);
int gwen_masked_l1_f32(const float *out, const float *target, const uint8_t *mask, int64_t members, int64_t N,
                       int64_t C, float *grad, float *loss, float *workspace, int64_t workspace_floats,
                       gwen_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Ensemble CRPS over the members axis, scores and gradient in one pass over the ensemble.
 * pred fp32 [M, N, C] (members first), target fp32 [N, C], both contiguous; node_w [N] >= 0 and chan_w [C] >= 0
 * or NULL (ones).  For a point with members x_1..x_M and truth y, k = pair_coef (alpha / (2M(M-1)) +
 * (1 - alpha) / (2M^2): alpha = 1 fair, 0 the ensemble's own CRPS):
 *     CRPS = (1/M) sum_i |x_i - y| - k sum_i sum_j |x_i - x_j|
 *     scores[0][c] = sum_n w_n CRPS(n,c) / sum w                      (per-channel CRPS)
 *     scores[1][c] = sum_n w_n (mean_i x_i - y)^2 / sum w             (RMSE^2 of the ensemble mean)
 *     scores[2][c] = sum_n w_n var_i(x_i) / sum w                     (spread^2; unbiased variance, NaN for M = 1)
 *     loss[0]      = sum_c v_c scores[0][c] / sum v
 *     grad_pred[i,n,c] = w_n v_c / (sum w sum v) * (sign(x_i - y) / M - 2k (#{x_j < x_i} - #{x_j > x_i}))
 *     grad_target[n,c] = -w_n v_c / (sum w sum v) / M * sum_i sign(x_i - y)              (sign(0) = 0)
 * grad_pred, grad_target and scores may be NULL; loss may not.  1 <= M <= 64, N >= 1, C >= 1, every pointer
 * 4-byte aligned, else GWEN_EINVAL before any HIP call (also for a workspace shorter than
 * gwen_ens_crps_workspace_floats(M, N, C) floats).  C % 4 == 0 with 16-byte aligned pred / target / grads reads
 * 16 bytes per lane.  Four launches, sums in a fixed order, no atomics (bitwise reproducible); zero weights give
 * NaN, as the expression does.
 * ------------------------------------------------------------------------------------------- */
int64_t gwen_ens_crps_workspace_floats(int64_t M, int64_t N, int64_t C);
int gwen_ens_crps_f32(const float *pred, const float *target, const float *node_w, const float *chan_w, int64_t M,
                      int64_t N, int64_t C, float pair_coef, float *grad_pred, float *grad_target, float *loss,
                      float *scores, float *workspace, int64_t workspace_floats, gwen_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The reference's ensemble losses (src/gwen/loss_functions.py), csrc/refloss.hip.  Everything is fp32, contiguous and
 * 4-byte aligned; offsets are 64-bit; 16 bytes per lane when every tensor is 16-byte aligned and R (the masked mean:
 * the element count, and inner for a row mask) is a multiple of 4, with the same bits as the 4-byte path.  No atomics,
 * sums in a fixed order (two runs are bitwise equal); no allocation, no synchronisation (the launches capture into a
 * hipGraph).  mu, sigma, z and the cdf stay in registers.  Errors come back before any HIP call: GWEN_EINVAL for a bad
 * size, M outside its range, S not dividing R, a flag that is not 0 / 1, a missing or misaligned pointer, or a workspace
 * shorter than the *_workspace_floats answer (0 for bad arguments); GWEN_ERANGE for more than 2^33 points A R (or
 * elements outer inner) or more than 2^40 elements A M R.
 *
 * Gaussian CRPS (CRPSLoss): pred [A, M, R], members in the middle (A = 1: the reference's dim = 0), target [A, R],
 * 2 <= M <= 256.  The A R points form consecutive samples of S points, S dividing R.  Per point, members x_1..x_M:
 *     mu = (1/M) sum_i x_i,   s = sqrt(sum_i (x_i - mu)^2 / (M - 1)),   sigma = s + 1e-6,
 *     z = (t - mu) / (sigma sqrt 2),   q = erf(z) / 2            (the normal cdf at t, minus 1/2)
 *     loss[sample] = (1/S) sum over its points of q^2                                         loss: [A R / S]
 * mu is evaluated as x_1 + (1/M) sum_i (x_i - x_1) (exact for identical members, no rounding of a common offset), and
 * deviations are formed about mu in a second sweep, never as E[x^2] - mu^2.  The backward takes grad_loss [A R / S]:
 *     c = grad_loss[sample] (2 q / S) exp(-z^2) / sqrt(pi)                                    (dL/dz)
 *     grad_target = c / (sigma sqrt 2)
 *     grad_pred_i = -c / (M sigma sqrt 2) - c (z / sigma) ds/dx_i,   ds/dx_i = (x_i - mu) / ((M - 1) s)
 * and ds/dx_i = 0 WHERE s == 0 (identical members), as torch's std backward.  grad_pred or grad_target may be NULL, not
 * both.  A NaN or Inf
 * member or target makes its own sample non-finite and no other.  workspace: 2 ceil(A R / 1024) floats.  The forward
 * reads pred once (above 32 members the second sweep reads the block's tile again), the backward reads it once and
 * writes grad_pred once.
 *
 * Variance-regularised L1 (EnsembleVarRegLoss): pred [A, M, R], target [A, M, R] (target_broadcast = 0) or [A, 1, R]
 * (1), M >= 1, value and gradients from one pass and a one-block finish:
 *     loss[0] = sum |x - t| / (A M R) - alpha sum_points var(x) / (A R),   var unbiased over the members
 *     grad_pred = sign(x - t) / (A M R) - alpha 2 (x_i - mu) / ((M - 1) A R)                  (sign(0) = 0)
 *     grad_target = -sign(x - t) / (A M R), summed over the members when the target is broadcast
 * grad_pred and grad_target may be NULL.  M = 1 gives NaN (value and grad_pred), as the expression does.
 * workspace: 2 ceil(A R / 1024) floats.
 *
 * Masked mean (MaskedLoss): out, target [outer, inner]; mask [inner] (mask_full = 0) or [outer, inner] (1), fp32;
 * kind GWEN_MASKED_L1: l = |out - target|, GWEN_MASKED_MSE: l = (out - target)^2:
 *     loss[0] = sum l mask / sum mask,     grad_out = l' mask / sum mask,     grad_target = -grad_out
 * where sum mask is the sum of the mask AS GIVEN ([inner] values when mask_full = 0), not of its broadcast: the
 * reference's expression.  An all-zero mask gives NaN, value and gradients.  grad_out and grad_target may be NULL.
 * workspace: 1025 + ceil(outer inner / 1024) floats.
 * ------------------------------------------------------------------------------------------- */
#define GWEN_MASKED_L1 0
#define GWEN_MASKED_MSE 1
int64_t gwen_gauss_crps_workspace_floats(int64_t A, int64_t M, int64_t R, int64_t S);
int gwen_gauss_crps_f32(const float *pred, const float *target, int64_t A, int64_t M, int64_t R, int64_t S,
                        float *loss, float *workspace, int64_t workspace_floats, gwen_stream_t stream);
int gwen_gauss_crps_bwd_f32(const float *grad_loss, const float *pred, const float *target, int64_t A, int64_t M,
                            int64_t R, int64_t S, float *grad_pred, float *grad_target, gwen_stream_t stream);
int64_t gwen_varreg_l1_workspace_floats(int64_t A, int64_t M, int64_t R);
int gwen_varreg_l1_f32(const float *pred, const float *target, int64_t A, int64_t M, int64_t R, int target_broadcast,
                       float alpha, float *grad_pred, float *grad_target, float *loss, float *workspace,
                       int64_t workspace_floats, gwen_stream_t stream);
int64_t gwen_masked_mean_workspace_floats(int64_t outer, int64_t inner);
int gwen_masked_mean_f32(const float *out, const float *target, const float *mask, int64_t outer, int64_t inner,
                         int mask_full, int kind, float *grad_out, float *grad_target, float *loss, float *workspace,
                         int64_t workspace_floats, gwen_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Ensemble products over the members axis (csrc/products.hip): per-point mean, spread, quantiles and exceedance
 * probabilities in ONE launch that reads every point once.  BUILD-DEFINED (the reference has none of these).
 * pred fp32 [M, N, C] (members first, contiguous), 1 <= M <= 64, N >= 1, C >= 1.  Every output is optional (NULL = not
 * wanted; Q = 0 / T = 0 likewise), at least one must be asked for.  For a point with members x_0..x_{M-1}:
 *     mean[n,c]  = r + (1/M) sum_i (x_i - r),  r = x_0            (differences to a member: no cancellation at offsets)
 *     std[n,c]   = sqrt(sum_i ((x_i - r) - dbar)^2 / (M - 1)),  dbar = (1/M) sum_i (x_i - r)
 *                  unbiased, from deviations about the mean, never E[x^2] - mean^2; M = 1 gives NaN, as torch
 *     quantiles[j,n,c], j < Q <= 32, q DEVICE fp32 [Q] in [0, 1]: numpy / torch "linear".  s = the members sorted
 *                  ascending, pos = q[j] (M - 1) rounded once in fp32, lo = floor(pos), frac = pos - lo;
 *                  frac == 0: s[lo], copied (q = 0 / 1 return the minimum / maximum, infinite ones too);
 *                  else s[lo] + frac (s[lo + 1] - s[lo]).  A q outside [0, 1] or NaN gives NaN.
 *     prob[t,n,c], t < T <= 32 = #{i : x_i > thr} / M, strict; thr DEVICE fp32 [T] (thr_per_channel = 0: thr[t]) or
 *                  [T, C] (thr_per_channel = 1: thr[t, c]).
 * NaN / Inf: a point with a NaN member has NaN in every quantile, in mean and in std, and no other point is touched;
 * prob counts a NaN member as not exceeding, as (pred > thr).float().mean(0).  +-Inf members sort as values; mean and
 * std of a point that has one are +-Inf or NaN, as the expressions above give.
 * Offsets are 64-bit.  C % 4 == 0 with 16-byte aligned pred / mean / std / prob, Q = 0 and M <= 16 reads 16 bytes per
 * lane (4 channels a thread); everything else 4 bytes per lane (quantiles sort one point per thread in registers);
 * every element is computed by the same operations on either path: the same bits.  One launch over persistent blocks
 * sized by occupancy, no workspace, no atomics, no allocation, no synchronisation.  Compulsory bytes:
 * 4 N C (M + Q + T + 2) with everything asked for.  Bad arguments (M, N, C, Q, T out of range, thr_per_channel not
 * 0 / 1, a missing or not 4-byte aligned pointer, nothing asked for) give GWEN_EINVAL before any HIP call.
 *
 * Rank (Talagrand) histogram of target fp32 [N, C] in pred: hist fp32 [C, M + 1].  For a point, b = #{i : x_i < y}
 * and t = #{i : x_i == y}: each of the bins b..b+t receives w_n / (t + 1) (the mid-rank split of ties: the
 * expectation of random tie-breaking).  node_w fp32 [N] or NULL (ones).  A point whose target or any member is NaN is
 * not counted; +-Inf compare as values.  normalize != 0 divides every channel's row by its own sum (a row that counted
 * nothing is NaN).  Two launches: per node chunk a partial histogram per channel, accumulated per thread in node order
 * and over the block's rows in row order (LDS), then a fixed-order sum over the chunks; no atomics, and the chunking is
 * a function of (M, N, C) alone, so two runs -- and runs on buffers of different alignment -- are bitwise equal.
 * workspace: gwen_ens_rank_hist_workspace_floats(M, N, C) = chunks * C * (M + 1) floats, with
 *     chunks = min(ceil(N / rows), 1024, max(1, 2^22 / (C (M + 1)))),  rows = threads / min(C, threads),
 *     threads = 256 (M <= 32) or 128:    at most 1024 chunks and at most 16 MiB (C (M + 1) floats if that is more).
 * Bad arguments, or a shorter workspace, give GWEN_EINVAL before any HIP call (the size function returns 0).
 * ------------------------------------------------------------------------------------------- */
int gwen_ens_products_f32(const float *pred, int64_t M, int64_t N, int64_t C, const float *q, int64_t Q,
                          const float *thr, int64_t T, int thr_per_channel, float *mean, float *std,
                          float *quantiles, float *prob, gwen_stream_t stream);
int64_t gwen_ens_rank_hist_workspace_floats(int64_t M, int64_t N, int64_t C);
int gwen_ens_rank_hist_f32(const float *pred, const float *target, const float *node_w, int64_t M, int64_t N,
                           int64_t C, int normalize, float *hist, float *workspace, int64_t workspace_floats,
                           gwen_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Latent noise: reproducible Gaussian noise per ensemble member, a pure function of
 *     z(seed, tag, draw, member, node, k),   k = channel of a noise vector.
 * Philox4x64-10 (numpy.random.Philox) with key = (seed, tag) and counter = (node, member, draw, k / 8), 64-bit words,
 * word 0 least significant.  The block's words w_0..w_3 split into h[2i] = lo32(w_i), h[2i+1] = hi32(w_i);
 * u_j = ((h_j >> 8) + 1/2) 2^-24 in (0, 1); Box-Muller on (u_2p, u_2p+1), p = 0..3:
 *     z[8 (k / 8) + 2p] = sqrt(-2 ln u_2p) cos(2 pi u_2p+1),    z[8 (k / 8) + 2p + 1] = sqrt(-2 ln u_2p) sin(2 pi u_2p+1).
 * (u needs 25 bits from 1/2 up: ln u is evaluated from 1 - u there, and the angle through sincospi of 2u or 2u - 2,
 * so that no argument is rounded.)  tag 0: latent noise; tag 1: initial-condition perturbation.
 * state: DEVICE uint64 [2] = {seed, draw}, 8-byte aligned, read by every launch (a captured hipGraph sees the current
 * draw on every replay).  No allocation, no synchronisation, no atomics.
 *
 *   gwen_noise_normal_f32: out[m, n, k] = z(state[0], tag, state[1], member0 + m, n, k), fp32 [members, nodes, K]
 *                          contiguous, any K >= 1.
 *   gwen_noise_inject_f32: out[r, :] = x[r, :] + sum_k z(state[0], 0, state[1], member0 + r / nodes, r % nodes, k) wz[:, k]
 *                          x, out fp32 [rows, H] (out may be x), wz fp32 [H, K] (an nn.Linear(K, H) weight); K in
 *                          {8, 16, 32, 64}, H % 4 == 0, x / out / wz 16-byte aligned.  The noise term is accumulated from
 *                          zero by fmaf in increasing k, then added to x: it does not depend on x or on any contraction
 *                          tier, and two launches are bitwise equal.
 *   gwen_noise_advance:    state[1] += n (n may be negative), one thread, in stream order.
 * Bad arguments give GWEN_EINVAL before any HIP call.
 * ------------------------------------------------------------------------------------------- */
int gwen_noise_normal_f32(const uint64_t *state, uint64_t tag, int64_t member0, int64_t members, int64_t nodes,
                          int64_t K, float *out, gwen_stream_t stream);
int gwen_noise_inject_f32(const uint64_t *state, int64_t member0, int64_t rows, int64_t nodes, const float *x,
                          const float *wz, int64_t H, int64_t K, float *out, gwen_stream_t stream);
int gwen_noise_advance(uint64_t *state, int64_t n, gwen_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Forcings (csrc/forcing.hip): inputs of the forecaster that it never predicts -- static fields (through `base`) and
 * functions of the valid time and the position -- added to the grid embedding in one launch.  BUILD-DEFINED.
 * clock: DEVICE int64 [2] = {t, dt}, 8-byte aligned: t seconds since 2000-01-01 00:00:00 UTC (may be negative), dt
 * seconds per step; read by every launch (a captured hipGraph sees the current time on every replay).
 * The solar vector of a point at latitude phi, longitude lambda (radians), AT the clock's t, with Y = 31 556 926 s and
 * mod the floor modulus on INTEGERS (t does not fit a float):
 *     gamma = 2 pi (t mod Y) / Y,     tau = 2 pi (t mod 86400) / 86400
 *     delta = 0.006918 - 0.399912 cos g + 0.070257 sin g - 0.006758 cos 2g + 0.000907 sin 2g - 0.002697 cos 3g
 *             + 0.00148 sin 3g                                                        (Spencer's series; g = gamma)
 *     E     = 0.000075 + 0.001868 cos g - 0.032077 sin g - 0.014615 cos 2g - 0.040849 sin 2g
 *     e0    = 1.000110 + 0.034221 cos g + 0.001280 sin g + 0.000719 cos 2g + 0.000077 sin 2g
 *     h     = tau + lambda + E - pi,     mu = sin phi sin delta + cos phi cos delta cos h
 *     f     = [e0 max(mu, 0), sin(tau + lambda), cos(tau + lambda), sin gamma, cos gamma]
 * evaluated in fp64 and rounded once to fp32.  No allocation, no synchronisation, no atomics.
 *
 *   gwen_forcing_advance:   clock[0] += n clock[1] (n may be negative), one thread, in stream order.
 *   gwen_forcing_solar_f32: out[n, :] = f(clock[0], latlon[n, 0], latlon[n, 1]); latlon double [N, 2] (lat, lon),
 *                           out fp32 [N, 5] contiguous.
 *   gwen_forcing_embed_f32: out[r, :] = x[r, :] + base[r % N, :] + sum_k f[r % N, k] wf[:, k]
 *                           f = the solar vector first (clock non-NULL; latlon is needed then), the Fg columns of
 *                           `given` (fp32 [N, Fg]; NULL with Fg = 0) after it; wf fp32 [H, 5 solar + Fg] (an nn.Linear
 *                           weight); base fp32 [N, H] or NULL; x, out fp32 [rows, H] (out may be x).  rows % N == 0
 *                           (rows / N members share latlon, given and base), H % 4 == 0, 1 <= 5 solar + Fg <= 64,
 *                           x / out / wf / base 16-byte aligned.  The forcing term is accumulated from zero by fmaf in
 *                           increasing k, then base is added, then x: it depends on no contraction tier and not on how
 *                           the members are batched, and two launches are bitwise equal.
 * Bad arguments give GWEN_EINVAL before any HIP call.
 * ------------------------------------------------------------------------------------------- */
int gwen_forcing_advance(int64_t *clock, int64_t n, gwen_stream_t stream);
int gwen_forcing_solar_f32(const int64_t *clock, const double *latlon, int64_t N, float *out, gwen_stream_t stream);
int gwen_forcing_embed_f32(const int64_t *clock, const double *latlon, const float *given, int64_t Fg, const float *wf,
                           const float *base, int64_t rows, int64_t N, const float *x, int64_t H, float *out,
                           gwen_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Edge attention (csrc/attention.hip): multi-head softmax attention of every target over its in-edges with an edge
 * term -- the kernel of gwen_amd.attention.GraphTransformer, forward and backward.  BUILD-DEFINED, PARITY UNPINNED (the
 * reference has no attention); PyG TransformerConv with edge_dim.  H heads, D = F / H, s(e) / d(e) the source / target of
 * stored edge e (edges stored by target: rowptr int32 [Nd + 1], src int32 [E]):
 *     sc[e,h]  = (1 / sqrt(D)) sum_{c in head h} q[d(e),c] (k[s(e),c] + ee[e,c])
 *     p[e,h]   = exp(sc[e,h] - lse[d(e),h]),   lse[d,h] = log sum_{e into d} exp(sc[e,h])
 *     out[d,c] = sum_{e into d} p[e,h(c)] (v[s(e),c] + ee[e,c])
 * in stored edge order, as a running-maximum ("online") softmax: no logit magnitude overflows.  A target without
 * in-edges gets out = 0 and lse = -inf.  ee [E, F] contiguous, in stored order, may be NULL (= 0).  fp32 throughout.
 * gwen_edge_attention_supported(F, H): F in {32, 64, 128, 256}, H a power of two, D >= 4.
 * q [Nd, F], k, v [Ns, F] with row strides ldq / ldk / ldv in floats (multiples of 4, >= F: column blocks of a
 * stacked projection); out, g [Nd, F] and lse [Nd, H] contiguous.  Feature pointers 16-byte aligned.  Row offsets are
 * 64-bit: no array has a size limit of its own; Nd, Ns or E >= 2^31 answer GWEN_ERANGE.  Outputs alias no input.
 *   gwen_edge_attention_f32:            out, lse.
 *   gwen_edge_attention_bwd_target_f32: pass T, one lane group per target; g = dL/dout, delta[d,h] = sum_{c in h} g out,
 *         dp[e,h] = sum_{c in h} g[d(e),c] (v[s(e),c] + ee[e,c]),   ds[e,h] = p[e,h] (dp[e,h] - delta[d(e),h]):
 *         gq[d] = (1 / sqrt(D)) sum_{e into d} ds[e,h] (k[s(e)] + ee[e])       [Nd, F] contiguous (0 without in-edges)
 *         gee[e] = (1 / sqrt(D)) ds[e,h] q[d(e)] + p[e,h] g[d(e)]              [E, F], written when ee is given
 *         P[e,h] = p, DS[e,h] = ds                                             [E, H] each, for pass S
 *   gwen_edge_attention_bwd_source_f32: pass S, one lane group per source over (src_rowptr int32 [Ns + 1], src_col
 *         int32 [E]: the stored positions of a source's out-edges, ascending) and dst int32 [E]:
 *         gk[s] = (1 / sqrt(D)) sum_{e out of s} ds[e,h] q[d(e)],   gv[s] = sum_{e out of s} p[e,h] g[d(e)]
 *         with row strides ldgk / ldgv (one [Ns, 2F] array may take both); a source without out-edges gets 0.
 * No atomics, fixed summation orders: two runs are bitwise equal.  Nothing allocates or synchronises (capturable).
 * Zero-sized calls (Nd == 0; Ns == 0 for pass S) return GWEN_OK before any HIP call; NULL or misaligned arguments
 * GWEN_EINVAL.  Non-finite inputs: a target whose in-edges (or own q row) carry +-Inf / NaN comes out non-finite in
 * that row of out / lse / gq and in those edges' rows of gee / P / DS (hence in gk / gv of their sources) only.
 * ------------------------------------------------------------------------------------------- */
int gwen_edge_attention_supported(int64_t F, int64_t H);
int gwen_edge_attention_f32(const float *q, int64_t ldq, const float *k, int64_t ldk, const float *v, int64_t ldv,
                            const float *ee, const int32_t *rowptr, const int32_t *src, int64_t Nd, int64_t Ns,
                            int64_t E, int64_t F, int64_t H, float *out, float *lse, gwen_stream_t stream);
int gwen_edge_attention_bwd_target_f32(const float *q, int64_t ldq, const float *k, int64_t ldk, const float *v,
                                       int64_t ldv, const float *ee, const int32_t *rowptr, const int32_t *src,
                                       const float *g, const float *out, const float *lse, int64_t Nd, int64_t Ns,
                                       int64_t E, int64_t F, int64_t H, float *gq, float *gee, float *P, float *DS,
                                       gwen_stream_t stream);
int gwen_edge_attention_bwd_source_f32(const int32_t *src_rowptr, const int32_t *src_col, const int32_t *dst,
                                       const float *q, int64_t ldq, const float *g, const float *P, const float *DS,
                                       int64_t Ns, int64_t Nd, int64_t E, int64_t F, int64_t H, float *gk, int64_t ldgk,
                                       float *gv, int64_t ldgv, gwen_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Grid graphs (csrc/gridgraph.hip): the grid <-> mesh graphs of the forecaster for arbitrary grid points.
 * BUILD-DEFINED, PARITY UNPINNED (the reference has no grid <-> mesh graphs: SURVEY section 0).  Positions are fp64
 * [n, 3] row-major, on (or near) the unit sphere: every coordinate in [-1, 1] (anything outside is clamped into the
 * outermost cell, so results stay correct, only slower).  A fixed-radius query runs through a uniform cell list over
 * [-1, 1]^3 with gwen_gridgraph_cells(R) = clamp(floor(2 / R), 1, 128) cells per axis (128: the dense cell-start table
 * is 8 MiB), points ordered by cell with one radix sort of unique 64-bit keys.  No atomics; two runs are bitwise equal.
 * radius must be finite and > 0 (GWEN_EINVAL); a count >= 2^31 - 1 is GWEN_ERANGE.
 *
 *   gwen_radius_edges_count: total int64 [1] (DEVICE) = the number of pairs (s, d) with
 *         (dx dx + dy dy) + dz dz <= R R,   (dx, dy, dz) = dst_pos[d] - src_pos[s],   fp64, in this association
 *         (no fused multiply-add), summed in 64 bits.  The larger of the two sets queries a cell list of the smaller
 *         (one thread per querying point); list and per-point offsets stay in `workspace`
 *         (gwen_radius_edges_workspace_bytes(num_src, num_dst)) for the fill.
 *   gwen_radius_edges_fill:  edge_index int64 [2, E] row-major (row 0 = s, row 1 = d), sorted by (d, s) ascending, and
 *         rowptr int32 [num_dst + 1] over it; E is the total the host read back, positions, sizes, radius and
 *         `workspace` are those of the count, untouched since; sort_workspace: gwen_radius_edges_fill_workspace_bytes(E).
 *         E >= 2^31 - 1 is GWEN_ERANGE; nothing is ever written at or beyond edge E.  E == 0 writes rowptr only.
 *   gwen_containing_faces:   for every point p the LOWEST face id f = (a, b, c) -- among the faces whose `centres` row is
 *         within `radius` of p by the expression above -- with det(p,b,c), det(p,c,a), det(p,a,b) all >= -1e-12, where
 *         det(u,v,w) = (u0 (v1 w2 - v2 w1) + u1 (v2 w0 - v0 w2)) + u2 (v0 w1 - v1 w0); weights fp64 [n, 3] = the three
 *         determinants over ((d0 + d1) + d2), so that sum_i w_i vertex_i is parallel to p.  face int32 [n] = -1 (weights 0)
 *         where no candidate contains p.  faces int64 [num_faces, 3] into mesh_pos [num_nodes, 3], positively oriented;
 *         a face with an index outside [0, num_nodes) contains nothing.
 *         workspace: gwen_containing_faces_workspace_bytes(num_faces).
 * ------------------------------------------------------------------------------------------- */
int gwen_gridgraph_cells(double radius);
int gwen_radius_edges_workspace_bytes(int64_t num_src, int64_t num_dst, size_t *bytes /* host */);
int gwen_radius_edges_count(const double *src_pos, int64_t num_src, const double *dst_pos, int64_t num_dst,
                            double radius, int64_t *total, void *workspace, size_t workspace_bytes,
                            gwen_stream_t stream);
int gwen_radius_edges_fill_workspace_bytes(int64_t E, size_t *bytes /* host */);
int gwen_radius_edges_fill(const double *src_pos, int64_t num_src, const double *dst_pos, int64_t num_dst,
                           double radius, int64_t E, int32_t *rowptr, int64_t *edge_index, const void *workspace,
                           size_t workspace_bytes, void *sort_workspace, size_t sort_workspace_bytes,
                           gwen_stream_t stream);
int gwen_containing_faces_workspace_bytes(int64_t num_faces, size_t *bytes /* host */);
int gwen_containing_faces(const double *points, int64_t n, const double *mesh_pos, int64_t num_nodes,
                          const int64_t *faces, const double *centres, int64_t num_faces, double radius,
                          int32_t *face, double *weights, void *workspace, size_t workspace_bytes,
                          gwen_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Regridding (csrc/regrid.hip): the exact k nearest source points of every target point on the unit sphere, and the
 * interpolation weights over them.  BUILD-DEFINED, PARITY UNPINNED (the reference moves no field between point sets).
 * Positions as for the grid graphs: fp64 [n, 3] unit vectors.  The search runs through the same cell list; no atomics, two
 * builds are bitwise equal.  1 <= k <= 8 (GWEN_EINVAL otherwise); sizes >= 2^31 - 1 are GWEN_ERANGE; bad arguments
 * return before any HIP call; num_rows == 0 returns 0.
 *
 *   Candidates of target t: the listed sources -- and, with max_distance D >= 0 (a chord length; negative: no limit),
 *         those with d2 <= D D -- where  d2 = (dx dx + dy dy) + dz dz  on  dst_pos[t] - src_pos[s],  fp64, in this
 *         association (no fused multiply-add).  A SOURCE MASK is applied before the call: list the unmasked sources only
 *         and pass their original indices as src_ids int32 [num_src] (NULL: a source reports its position in the list).
 *   Row t:  its min(k, candidates) candidates in ascending (d2, reported index) order, compared lexicographically: the
 *         lowest index wins every tie.  idx int32 [num_dst, k] padded with -1, d2 fp64 [num_dst, k] padded with +inf,
 *         count int32 [num_dst] = min(k, candidates).
 *   gwen_knn_query: ONE ROUND of the search at `radius` R (finite, > 0) for the targets `rows` (int32 [num_rows], each
 *         in [0, num_dst); NULL: all targets, num_rows == num_dst).  One thread per row keeps its k best within R.  A
 *         row with at least k candidates within R is final -- everything outside R is farther -- and is written; a row
 *         with fewer is NOT written: its id goes to next_rows (int32, room for num_rows; row order kept) and
 *         next_count int32 [1] (DEVICE) counts them.  The caller reads next_count back, doubles R and calls again with
 *         rows = next_rows (another buffer).  A call with R >= D or R >= 2 (the whole sphere) writes every row it is
 *         given and sets next_count = 0, so the loop ends; the result does not depend on the first R.
 *         workspace: gwen_knn_workspace_bytes(num_src, num_dst).
 *         A pole row of a lat-lon source is nlon coincident points in one cell: a target next to the pole walks all of
 *         them.  This is accepted.
 *   gwen_knn_weights: weights fp32 [num_dst, k] (0 in the padding) and entries int32 [num_dst] from d2 / count above,
 *         computed in fp64 and rounded once.  GWEN_REGRID_IDW: w_j = u_j / ((u_0 + u_1) + ...) with u = d^-power,
 *         d = sqrt(d2); power 1 and 2 are 1 / sqrt(d2) and 1 / d2 (no pow); power finite and > 0.  COINCIDENCE: a row whose
 *         nearest d2 <= 1e-24 becomes ONE entry (entries = 1) of weight exactly 1.0f, so a NaN in a neighbour never reaches
 *         a target that sits on a source.  GWEN_REGRID_NEAREST: one entry of weight 1.0f.  entries = 0 where count = 0.
 * ------------------------------------------------------------------------------------------- */
#define GWEN_REGRID_NEAREST 0
#define GWEN_REGRID_IDW 1
int gwen_knn_workspace_bytes(int64_t num_src, int64_t num_dst, size_t *bytes /* host */);
int gwen_knn_query(const double *src_pos, const int32_t *src_ids, int64_t num_src, const double *dst_pos,
                   int64_t num_dst, const int32_t *rows, int64_t num_rows, int k, double radius, double max_distance,
                   int32_t *idx, double *d2, int32_t *count, int32_t *next_rows, int32_t *next_count,
                   void *workspace, size_t workspace_bytes, gwen_stream_t stream);
int gwen_knn_weights(const double *d2, const int32_t *count, int64_t num_dst, int k, int method, double power,
                     float *weights, int32_t *entries, gwen_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Conservative regridding (csrc/conserve.hip): the overlap areas of two sets of cells on the unit sphere and the
 * first-order conservative weights from them.  BUILD-DEFINED, PARITY UNPINNED (the reference regrids nothing); restated
 * in numpy in tests/conserve_ref.py.  No launcher allocates, synchronises or uses atomics; two builds are bitwise equal.
 * 3 <= V <= 8 and a valid mode (GWEN_EINVAL otherwise); sizes >= 2^31 - 1 are GWEN_ERANGE; bad arguments return before any
 * HIP call; an empty problem returns 0.
 *
 *   GEOMETRY.  A cell is a CONVEX spherical polygon: V vertices, unit vectors, counter-clockwise seen from outside, joined
 *         by GREAT-CIRCLE arcs, inside a cap of chord radius <= 1 about its normalised vertex mean.  A cell set is fp64
 *         [N, V, 3] row-major.  A cell with fewer corners repeats a vertex (a lat-lon cell at a pole is a wedge whose two
 *         polar corners coincide); an edge whose two ends are equal in every coordinate is SKIPPED, never clipped against.
 *         A lat-lon box gets great-circle edges where the true box has parallels; neighbours share the same arc, so the
 *         cells still tile the sphere exactly.  All of it is fp64 without fused multiply-add:
 *             dot(a, b)     = (a0 b0 + a1 b1) + a2 b2
 *             cross(a, b)   = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0)
 *             tri(a, b, c)  = 2 atan2(dot(a, cross(b, c)), ((1 + dot(a, b)) + dot(b, c)) + dot(c, a))
 *             area(P)       = (tri(P0, P1, P2) + tri(P0, P2, P3)) + ...      0 with fewer than 3 vertices
 *   OVERLAP of source cell S and target cell T: S, clipped in turn against the half-space dot(cross(a, b), p) >= 0 of every
 *         non-degenerate edge (a, b) = (T_j, T_j+1) of T, j ascending (Sutherland-Hodgman in 3-D: walking the arcs (p, q)
 *         of the polygon from vertex 0, an inside p is kept, and where p and q lie on different sides the crossing
 *         |d_p| q + |d_q| p, divided by its length, follows); then area().  At most 16 vertices are held, which every
 *         convex input respects; a 17th is dropped.
 *   KEEP RULE (applied by the caller): a pair is an entry when area > 1e-12 min(A_S, A_T).  Cells that only share an edge
 *         or a corner give slivers of relative size <= 4e-15; the cut sits far above them and far below any real overlap.
 *
 *   gwen_cell_areas: per cell, centre fp64 [n, 3] = s / sqrt(dot(s, s)) with s = ((v_0 + v_1) + v_2) + ..., radius fp64 [n]
 *         = sqrt of the largest (dx dx + dy dy) + dz dz over d = v_k - centre, area fp64 [n] = area(cell).
 *   gwen_cell_overlap_areas: one work item per candidate pair; pairs int64 [2, e] row-major (row 0 = source cell, row 1 =
 *         target cell; an index out of range gives area 0).  A pair with (dx dx + dy dy) + dz dz > (r_S + r_T)(r_S + r_T)
 *         on d = dst_centre - src_centre is rejected (the caps are disjoint, so are the cells), else clipped and measured.
 *         area fp64 [e]: 0 for a rejected or empty pair (a sliver may come out as a tiny negative number).
 *   gwen_cell_overlap_weights: rowptr int64 [num_dst + 1] over the kept pairs (sorted by target), area fp64 [e] their
 *         areas, dst_area fp64 [num_dst].  One thread per target sums its row in stored order in fp64:
 *         coverage fp64 [num_dst] = sum / A_t; weights fp32 [e] = A_ts / sum (GWEN_CONSERVE_COVERED: a constant stays
 *         constant on a partially covered target) or A_ts / A_t (GWEN_CONSERVE_CELL: the integral is preserved), computed
 *         in fp64 and rounded once.
 * ------------------------------------------------------------------------------------------- */
#define GWEN_CONSERVE_COVERED 0
#define GWEN_CONSERVE_CELL 1
int gwen_cell_areas(const double *cells, int64_t n, int v, double *centre, double *radius, double *area,
                    gwen_stream_t stream);
int gwen_cell_overlap_areas(const double *src_cells, int64_t num_src, int vs, const double *dst_cells, int64_t num_dst,
                            int vt, const int64_t *pairs, int64_t e, const double *src_centre, const double *src_radius,
                            const double *dst_centre, const double *dst_radius, double *area, gwen_stream_t stream);
int gwen_cell_overlap_weights(const int64_t *rowptr, const double *area, const double *dst_area, int64_t num_dst,
                              int64_t e, int mode, float *weights, double *coverage, gwen_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Spherical harmonic transforms on a latitude-longitude grid (csrc/sht.hip, gwen_amd.spectral).
 *
 *   x [batch, nlat * nlon, C]: rows (lat, lon) row-major, south to north, longitude 2 pi i / nlon.
 *   coef [batch, (lmax + 1)^2, C]: row l^2 + l + m holds (l, m); m >= 0 goes with cos m lon, m < 0 with sin |m| lon.
 *   Basis: real, 4 pi-normalised, Y_lm = Pbar_l^|m|(sin lat) {cos, sin}(|m| lon), sphere mean of Y^2 = 1, with
 *         Pbar_m^m = seed[m] cos^m lat,  Pbar_l^m = a (sin lat Pbar_{l-1}^m - b Pbar_{l-2}^m),
 *         a = sqrt((4 l^2 - 1) / (l^2 - m^2)),  b = sqrt(((l - 1)^2 - m^2) / (4 (l - 1)^2 - 1)),
 *         generated in the kernels; nothing of size [m, l, lat] is ever stored.
 *   Tables, all fp64 on the device: nodes [nlat, 2] = (sin lat, cos lat), 16-byte aligned; twiddle [nlon, 2] =
 *         (cos, sin)(2 pi i / nlon), 16-byte aligned (the kernels index it by (m i) mod nlon and never call cos);
 *         seed [lmax + 1], seed[0] = 1, seed[1] = sqrt 3, seed[m] = seed[m - 1] sqrt((2m + 1) / (2m)) from m = 2;
 *         lat_w [nlat] or NULL (= ones): the latitude weight.
 *
 *   gwen_sht_analysis:  coef_lm = sum_j lat_w[j] Pbar_l^m(j) sum_i x[j, i] {cos, sin}(m lon_i).  With lat_w = the
 *         quadrature weight over nlon it is the analysis; with NULL it is the adjoint of the synthesis.
 *   gwen_sht_synthesis: x[j, i] = lat_w[j] sum_lm coef_lm Y_lm(j, i).  With NULL it is the synthesis; with the
 *         quadrature weights it is the adjoint of the analysis.
 *   x and coef are fp32 (x_f64 / coef_f64 = 0) or fp64 (1), inputs and outputs alike.  Every sum is accumulated in fp64
 *   by one thread in index order; no atomics; results are bitwise equal run to run, whatever the batch, an item's place
 *   in it or the workspace size.  A non-finite input stays in its (item, channel).
 *   workspace: the fp64 ring sums [chunk, nlat, 2 lmax + 1, C]; gwen_sht_workspace_bytes() is the size of ONE item
 *         (0 for bad sizes) and the batch is cut into chunks of workspace_bytes / that many items (GWEN_ENOSPACE
 *         below one item).  8-byte aligned.
 *   grid: which quadrature the sizes are checked against -- lmax <= (nlat - 1) / 2 on the equiangular grids,
 *         lmax <= nlat - 1 on the Gauss grid.  Always nlon >= 2 lmax + 1, lmax <= 1023, nlat <= 2048.  A bad grid, size
 *         or flag, a missing or misaligned pointer: GWEN_EINVAL; nlat nlon or C >= 2^31: GWEN_ERANGE; both before any HIP
 *         call.  batch == 0 returns 0.  Element offsets are 64-bit.
 *   gwen_sht_power_f64: power [batch, lmax + 1, C] fp64, S_l = sum_m coef_lm^2 in the order m = -l ... l.
 *
 *   Vector harmonics, on the unit sphere: u [batch, nlat * nlon, C] is the eastward and v the northward component, vort
 *   and div [batch, (lmax + 1)^2, C] the spectral vorticity and divergence, rows as coef.  With streamfunction psi and
 *   velocity potential chi,
 *         u = -d psi/d lat + (1 / cos lat) d chi/d lon,   v = (1 / cos lat) d psi/d lon + d chi/d lat,
 *         vort = lap psi,  div = lap chi,  lap Y_lm = -L Y_lm,  L = l (l + 1).
 *   With Q_l^m = Pbar_l^m / cos lat and D_l^m = d Pbar_l^m / d lat, grad Y of the cos row (l, m >= 0) is (east, north) =
 *   (-m Q sin m lon, D cos m lon), of the sin row (l, -m) it is (m Q cos m lon, D sin m lon), and k x grad Y =
 *   (-north, east) of grad Y.  The kernels never divide by cos lat (pole rows are ordinary rows): for m >= 1, Q_l^m walks
 *   the recurrence of Pbar_l^m from seed[m] cos^(m-1) lat and D_l^m = -l sin lat Q_l^m + sqrt((2l + 1)(l^2 - m^2) /
 *   (2l - 1)) Q_{l-1}^m; for m = 0 the Q term carries the factor m = 0 and D_l^0 = sqrt(l (l + 1) / 2) Pbar_l^1.
 *   gwen_sht_vector_synthesis: (u, v)[j, i] = lat_w[j] sum_lm psi_lm (k x grad Y_lm) + chi_lm grad Y_lm, with psi_lm =
 *         -vort_lm / L and chi_lm = -div_lm / L (adjoint = 0) or psi_lm = -vort_lm, chi_lm = -div_lm (adjoint = 1).  Row 0
 *         is read as 0 whatever it holds; vort or div (not both) may be NULL, meaning zero.  lat_w = NULL, adjoint = 0:
 *         the synthesis.  lat_w = the quadrature weights, adjoint = 1: the adjoint of the analysis.
 *   gwen_sht_vector_analysis: div_lm = -s_l sum_p lat_w (u, v) . grad Y_lm and vort_lm = -s_l sum_p lat_w (u, v) .
 *         (k x grad Y_lm), with s_l = 1 (adjoint = 0) or 1 / L (adjoint = 1); row 0 is stored as 0.  lat_w = the
 *         quadrature weights, adjoint = 0: the analysis, the inverse of the synthesis on band-limited pairs.  lat_w =
 *         NULL, adjoint = 1: the adjoint of the synthesis.
 *   u, v share x_f64 and vort, div share coef_f64.  Tables, sums, reproducibility and errors are those of the scalar
 *   entries; adjoint outside {0, 1} is GWEN_EINVAL.  workspace: the ring sums of u and of v, [2, chunk, nlat,
 *   2 lmax + 1, C] fp64; gwen_sht_vector_workspace_bytes() is the size of ONE item (twice the scalar's, 0 for bad sizes).
 * ------------------------------------------------------------------------------------------- */
#define GWEN_SHT_EQUIANGULAR 0
#define GWEN_SHT_EQUIANGULAR_CENTRED 1
#define GWEN_SHT_GAUSS 2
int64_t gwen_sht_workspace_bytes(int grid, int64_t nlat, int64_t nlon, int64_t lmax, int64_t C);
int gwen_sht_analysis(const void *x, int x_f64, void *coef, int coef_f64, const double *nodes, const double *lat_w,
                      const double *twiddle, const double *seed, int grid, int64_t batch, int64_t nlat, int64_t nlon,
                      int64_t lmax, int64_t C, void *workspace, size_t workspace_bytes, gwen_stream_t stream);
int gwen_sht_synthesis(const void *coef, int coef_f64, void *x, int x_f64, const double *nodes, const double *lat_w,
                       const double *twiddle, const double *seed, int grid, int64_t batch, int64_t nlat, int64_t nlon,
                       int64_t lmax, int64_t C, void *workspace, size_t workspace_bytes, gwen_stream_t stream);
int gwen_sht_power_f64(const double *coef, double *power, int64_t batch, int64_t lmax, int64_t C,
                       gwen_stream_t stream);
int64_t gwen_sht_vector_workspace_bytes(int grid, int64_t nlat, int64_t nlon, int64_t lmax, int64_t C);
int gwen_sht_vector_analysis(const void *u, const void *v, int x_f64, void *vort, void *div, int coef_f64,
                             const double *nodes, const double *lat_w, const double *twiddle, const double *seed,
                             int grid, int64_t batch, int64_t nlat, int64_t nlon, int64_t lmax, int64_t C, int adjoint,
                             void *workspace, size_t workspace_bytes, gwen_stream_t stream);
int gwen_sht_vector_synthesis(const void *vort, const void *div, int coef_f64, void *u, void *v, int x_f64,
                              const double *nodes, const double *lat_w, const double *twiddle, const double *seed,
                              int grid, int64_t batch, int64_t nlat, int64_t nlon, int64_t lmax, int64_t C, int adjoint,
                              void *workspace, size_t workspace_bytes, gwen_stream_t stream);

/* One entry for the four transforms above, and the choice of the longitude stage.
 *
 *   op: which transform.  in0 (in1) and out0 (out1) are its inputs and outputs in the order of the entry above -- x and
 *         coef, or (u, v) and (vort, div); the scalar transforms ignore in1, out1 and adjoint.  in_f64 / out_f64 are the
 *         dtype flags of the inputs and of the outputs.  Every other field is the argument of that name.
 *   longitude: GWEN_SHT_LON_DIRECT, the direct sums of the four entries above (which are this call with it, bit for bit),
 *         or GWEN_SHT_LON_FFT: every latitude ring of every channel is one fp64 mixed-radix FFT (radices 4, 2, 3, 5) in
 *         LDS, of length nlon / 2 and a split step when nlon is even, of length nlon when it is odd; every twiddle is an
 *         entry of the same nlon-entry table.  Orders above lmax are not stored and read as zero.  The ring sums, the
 *         workspace and the latitude kernels are the same; results agree with the direct sums to rounding (not bit for
 *         bit: the order of the additions differs) and are as reproducible: fixed by one item's, one latitude's and one
 *         channel's inputs and by nlon, whatever the batch, the chunking or the run; a non-finite input stays in its
 *         (item, channel).  gwen_sht_fft_supported(nlon): 1 iff 1 <= nlon <= 4096 and nlon = 2^a 3^b 5^c (no HIP call).
 *   A NULL call, an unknown op or longitude, GWEN_SHT_LON_FFT with an nlon it does not support: GWEN_EINVAL; every other
 *   error as the entries above, all before any HIP call. */
#define GWEN_SHT_OP_ANALYSIS 0
#define GWEN_SHT_OP_SYNTHESIS 1
#define GWEN_SHT_OP_VECTOR_ANALYSIS 2
#define GWEN_SHT_OP_VECTOR_SYNTHESIS 3
#define GWEN_SHT_LON_DIRECT 0
#define GWEN_SHT_LON_FFT 1
typedef struct gwen_sht_call {
  int32_t op;        /* GWEN_SHT_OP_* */
  int32_t longitude; /* GWEN_SHT_LON_* */
  const void *in0, *in1;
  int32_t in_f64;
  void *out0, *out1;
  int32_t out_f64;
  const double *nodes, *lat_w, *twiddle, *seed;
  int32_t grid, adjoint;
  int64_t batch, nlat, nlon, lmax, C;
  void *workspace;
  size_t workspace_bytes;
  gwen_stream_t stream;
} gwen_sht_call;
int gwen_sht_transform(const gwen_sht_call *call);
int gwen_sht_fft_supported(int64_t nlon);

/* ---------------------------------------------------------------------------------------------
 * Spherical harmonic transforms on a reduced Gaussian grid (csrc/sht.hip, gwen_amd.spectral.SphericalHarmonics.reduced):
 * the nlat Gauss-Legendre latitudes, south to north, with a ring length of its own on every latitude (the octahedral and
 * the classic reduced grids of IFS, ERA5, AIFS).  Basis, coefficient rows, ops, dtype flags, lat_w, adjoint, workspace
 * layout, chunking, reproducibility and NaN containment are those of gwen_sht_transform; the latitude kernels are the same.
 *
 *   ring_nlon [nlat] int32: ring j holds the longitudes 2 pi i / ring_nlon[j], i = 0 ... ring_nlon[j] - 1.
 *   ring_start [nlat + 1] int64, 8-byte aligned: ring_start[j] = sum_{k < j} ring_nlon[k]; ring_start[nlat] = points.
 *   x (u, v) [batch, points, C]: rows ring-major, row ring_start[j] + i is longitude i of ring j.
 *   twiddle [points, 2] fp64, 16-byte aligned: one table a ring, end to end, twiddle[ring_start[j] + i] =
 *         (cos, sin)(2 pi i / ring_nlon[j]); ring j indexes its own by (m i) mod ring_nlon[j].
 *   nodes, seed, lat_w: as above; the quadrature weight of ring j is w_j / ring_nlon[j].
 *   max_nlon: the longest ring.  Sizes: 1 <= nlat <= 2048, 0 <= lmax <= min(1023, nlat - 1), max_nlon >= 2 lmax + 1,
 *         nlat - 1 + max_nlon <= points <= nlat max_nlon, points < 2^31.  Element offsets are 64-bit.
 *   Truncation: ring j carries the orders m <= M_j = min(lmax, (ring_nlon[j] - 1) / 2).  The longitude sums of an
 *         analysis store zeros in the workspace columns of the orders above M_j (the workspace may arrive holding
 *         anything); those of a synthesis do not read them.  Both are one masked operator, so lat_w and adjoint give the
 *         adjoints as they do above.  Where every ring_nlon[j] >= 2 lmax + 1 nothing is truncated, and rings of one
 *         length nlon give the bits of gwen_sht_transform(GWEN_SHT_GAUSS, GWEN_SHT_LON_DIRECT) on nlat x nlon.
 *   The longitude stage is always the direct sums: one thread's fp64 fma chain in ascending i (analysis) or m (synthesis).
 *   The scalar fields are validated before any HIP call -- GWEN_EINVAL for a bad size, flag or op, a NULL call, a missing
 *   or misaligned pointer (the two ring tables included); GWEN_ERANGE for points, max_nlon or C >= 2^31; GWEN_ENOSPACE
 *   for a workspace below one item.  The CONTENTS of the device tables are the caller's responsibility: ring lengths that
 *   do not add up to ring_start, a length above max_nlon or a start beyond points make the kernels read and write out
 *   of bounds.  gwen_sht_rings_workspace_bytes(vector, ...): the size of ONE item of a scalar (vector = 0) or a vector
 *   (1) transform, 0 for bad sizes.
 * ------------------------------------------------------------------------------------------- */
typedef struct gwen_sht_rings_call {
  int32_t op;      /* GWEN_SHT_OP_* */
  int32_t adjoint; /* the vector transforms' flag; the scalar ones ignore it */
  const void *in0, *in1;
  int32_t in_f64;
  void *out0, *out1;
  int32_t out_f64;
  const double *nodes, *lat_w, *twiddle, *seed;
  const int32_t *ring_nlon;
  const int64_t *ring_start;
  int64_t batch, nlat, points, max_nlon, lmax, C;
  void *workspace;
  size_t workspace_bytes;
  gwen_stream_t stream;
} gwen_sht_rings_call;
int gwen_sht_rings_transform(const gwen_sht_rings_call *call);
int64_t gwen_sht_rings_workspace_bytes(int vector, int64_t nlat, int64_t points, int64_t max_nlon, int64_t lmax,
                                       int64_t C);

/* The same transforms with one fp64 FFT a ring, item and channel in LDS as the longitude stage, whatever the ring's length
 * (csrc/sht_fft.h; gwen_amd.spectral, ring_longitude="bluestein").  `rings` is the call above, field for field: the
 * tables, the truncation, the workspace (gwen_sht_rings_workspace_bytes) and the latitude kernels are the same, and the
 * results agree with gwen_sht_rings_transform to rounding.
 *
 *   gwen_sht_ring_fft_plan(nlon, &n, &M): how a ring of nlon longitudes runs -- n = nlon / 2 for an even nlon (the FFT of
 *         z[k] = x[2k] + i x[2k + 1] and a split step), n = nlon for an odd one.  1 (mixed): gwen_sht_fft_supported(nlon),
 *         the radix-4/2/3/5 FFT of gwen_sht_transform(GWEN_SHT_LON_FFT) on the ring's own slice of `twiddle`, M = 0; rings
 *         of one such length give the bits of that call on GWEN_SHT_GAUSS.  2 (Bluestein): any other nlon, as a cyclic
 *         convolution of length M, the smallest 2^a 3^b 5^c >= 2 n - 1, where M <= 4096.  0: no such M (or nlon < 1, or a
 *         NULL n or M), the ring is not supported.  No HIP call.
 *   ring_plan [nlat, 8] int32, 16-byte aligned: (kind, n, M, chirp_at, filter_at, conv_at, 0, 0) of ring j -- the three
 *         numbers above and, for a Bluestein ring, the complex entry at which its slices of the three tables start.
 *   chirp [*, 2] fp64: a slice of n entries, c_k = exp(-i pi k^2 / n) as (re, im).
 *   filter [*, 2] fp64: a slice of M entries, H = FFT_M(h) / M (forward, exp(-i ...)) of h_k = conj c_k at k = 0 ... n - 1
 *         and at M - k, zero elsewhere.  The synthesis uses conj c and conj H.
 *   conv_twiddle [*, 2] fp64: a slice of M entries, (cos, sin)(2 pi k / M).  All three 16-byte aligned, never NULL (a
 *         grid of mixed rings alone passes tables that nothing reads).
 *   max_points: the largest of n (mixed rings) and M (Bluestein rings), 1 ... 4096: it sizes the grid and the LDS.
 *   Reproducibility and NaN containment as gwen_sht_transform(GWEN_SHT_LON_FFT): nothing is packed across channels, the
 *   schedule of a ring is fixed by its length, no atomics.  Errors as gwen_sht_rings_transform, with GWEN_EINVAL for a
 *   max_points out of range and for a missing or misaligned ring_plan or table, all before any HIP call.  The CONTENTS
 *   of ring_plan are the caller's responsibility as those of the ring tables are; a block whose record does not fit
 *   its ring's length or the launch's LDS stores nothing. */
typedef struct gwen_sht_rings_fft_call {
  gwen_sht_rings_call rings;
  const int32_t *ring_plan;
  const double *chirp, *filter, *conv_twiddle;
  int64_t max_points;
} gwen_sht_rings_fft_call;
int gwen_sht_rings_fft_transform(const gwen_sht_rings_fft_call *call);
int gwen_sht_ring_fft_plan(int64_t nlon, int64_t *n, int64_t *M);

/* ---------------------------------------------------------------------------------------------
 * Spectral convolution (csrc/spectral_conv.hip, gwen_amd.sfno): the learned map of a spherical Fourier neural operator.
 *
 *   coef [batch, T, Cin], T = (lmax + 1)^2, rows as the transforms above: degree l owns rows l^2 .. l^2 + 2l.
 *   W [lmax + 1, Cin, Cout]: one real matrix a degree, shared by every m (a zonal filter: the map commutes with every
 *         rotation of the sphere).  out [batch, T, Cout].  Everything fp32, contiguous, 16-byte aligned.
 *
 *   gwen_spectral_conv_f32: out[b, l^2 + j, :] = coef[b, l^2 + j, :] . W[l], 0 <= j <= 2l.  With transpose_w = 1 the
 *         product is with W[l]^T and W is read as stored [lmax + 1, Cout, Cin] -- the gradient in coef of the forward
 *         whose weight it is, without a transposing copy.  out must not alias coef.
 *   gwen_spectral_conv_grad_weight_f32: grad_W[l] = sum_b sum_j coef[b, l^2 + j, :]^T g[b, l^2 + j, :], g [batch, T,
 *         Cout], grad_W [lmax + 1, Cin, Cout]; summed b outer, j inner by the one block that owns the tile: no atomics.
 *   gwen_spectral_conv_supported: 1 where Cin and Cout are multiples of 16 in [16, 512] and contract is a split
 *         contraction -- GWEN_CONTRACT_BF16X6 (fp32-class; GWEN_CONTRACT_F16X3 means it here, as in K3) or
 *         GWEN_CONTRACT_BF16X3 -- else 0.  There is no fp32-input-MFMA and no fp64 path.
 *   W[l] is cut into bf16 images on the fly (split.h), fp32 accumulators in ascending k.  Results are bitwise equal run
 *   to run; in the forward an item's rows are the same bits whatever the batch and the other items.  Element offsets are
 *   64-bit.  Unsupported sizes, batch < 0, lmax outside [0, 1023], a flag outside {0, 1}, a missing or misaligned
 *   pointer: GWEN_EINVAL; batch (2 lmax + 1) >= 2^31: GWEN_ERANGE; both before any HIP call.  batch == 0 returns 0 and
 *   writes nothing.  No host synchronisation.
 * ------------------------------------------------------------------------------------------- */
int gwen_spectral_conv_supported(int64_t Cin, int64_t Cout, int contract);
int gwen_spectral_conv_f32(const float *coef, const float *W, float *out, int64_t batch, int64_t lmax, int64_t Cin,
                           int64_t Cout, int transpose_w, int contract, gwen_stream_t stream);
int gwen_spectral_conv_grad_weight_f32(const float *coef, const float *g, float *grad_W, int64_t batch, int64_t lmax,
                                       int64_t Cin, int64_t Cout, int contract, gwen_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * U-Net kernels (csrc/conv.hip, gwen_amd.models_cnn).  Activations are channels-last fp32: [B, H, W, C] is a row matrix
 * [B H W, C] with a row pitch ld >= C (in elements), so a kernel reads or writes a channel slice of a wider buffer.
 *
 *   gwen_conv3x3_pack_f32: W -> the bf16 fragment images gwen_conv3x3_f32 reads, gwen_conv3x3_pack_bytes(Cin, Cout,
 *         contract) bytes (0 for unsupported arguments), 16-byte aligned: [Cin chunk of 32][tap ky 3 + kx][tile of 16
 *         output channels][image][lane][8], channels beyond Cin / Cout as zeros.  transposed = 0: Conv2d weights
 *         [Cout, Cin, 3, 3]; transposed = 1: ConvTranspose2d weights [Cin, Cout, 3, 3], which at stride 1 and
 *         padding 1 is the convolution with Wc[co][ci][ky][kx] = Wt[ci][co][2 - ky][2 - kx].  One launch, on the device.
 *   gwen_conv3x3_f32: out[b, y, x, co] = sum_{ky, kx, ci} Wc[co][ci][ky][kx] x[b, y + ky - 1, x + kx - 1, ci] (zero
 *         outside the image) + bias[co] (bias may be NULL), as an implicit GEMM on a split contraction:
 *         GWEN_CONTRACT_BF16X6 (fp32-class; GWEN_CONTRACT_F16X3 means it here, as in K3) or GWEN_CONTRACT_BF16X3, which
 *         must be the one the image was packed for.  flags, a sum of
 *           GWEN_CONV_POOL    2x2 / stride 2 max-pool of (conv + bias), floor rule: out is [B, H / 2, W / 2, Cout]
 *                             and the un-pooled result is never written; a NaN in a window gives NaN;
 *           GWEN_CONV_AFFINE  then v scale[co] + shift[co]  (after the pool: a negative scale does not commute with max);
 *           GWEN_CONV_RELU    then max(0, v).
 *         1 <= Cin, Cout <= 2048.  Channels beyond Cin and pixels outside the image enter as true zeros, whatever
 *         the memory there holds.  out must not overlap x.  Where one image gives too few blocks to fill the chip
 *         (low resolutions, many channels) Cin is cut into up to 16 slices, one block each, whose raw sums
 *         [slice][B H W][Cout] go through workspace and are added in slice order by a second launch, which applies the
 *         epilogue: gwen_conv3x3_workspace_floats(B, H, W, Cin, Cout, flags) floats (0: one launch, workspace may be
 *         NULL; -1: the slices' sums would reach 4 GiB and gwen_conv3x3_f32 answers GWEN_ERANGE; a shorter workspace:
 *         GWEN_ENOSPACE).  The cut depends on H, W, Cin, Cout and the pool flag only; gwen_conv3x3_plan reports it
 *         (output-channel tiles of 16 per block, 1 .. 4, and slices of Cin, 1 .. 16) -- the launcher and the size
 *         function read the same plan, and a split never runs without its workspace.  More than 2^24 - 1 pixel
 *         tiles of 8 x 16 in a batch: GWEN_ERANGE.
 *   gwen_upsample2x_f32: bilinear x 2 with align_corners = True (source position o (n - 1) / (2 n - 1); n = 1 copies),
 *         out [B, 2 Hin, 2 Win, C], then the affine and ReLU of flags (GWEN_CONV_AFFINE, GWEN_CONV_RELU).
 *   gwen_channel_stats_f64: mean[c] and the biased variance var[c] of the rows of x [rows, C] (pitch ld), from sums
 *         of x and x^2 in fp64, added in a fixed order in two stages (row chunks, then the chunks); workspace of
 *         gwen_channel_stats_workspace_bytes(rows, C) bytes, 8-byte aligned (GWEN_ENOSPACE if shorter).  rows >= 1.
 *   gwen_affine_relu_f32: x[r, c] = max(0, x[r, c] scale[c] + shift[c]) in place.
 *
 * No atomics, 64-bit element offsets, results bitwise equal run to run; in gwen_conv3x3_f32 and gwen_upsample2x_f32 an
 * image's output has the same bits whatever the batch around it.  Bad sizes, flags, contracts (GWEN_CONTRACT_F32
 * included), missing or misaligned pointers: GWEN_EINVAL; an input or output of 4 GiB or more: GWEN_ERANGE; both
 * before any HIP call.  Empty outputs return GWEN_OK and write nothing.  No host synchronisation.
 * ------------------------------------------------------------------------------------------- */
#define GWEN_CONV_AFFINE 1
#define GWEN_CONV_RELU 2
#define GWEN_CONV_POOL 4
int64_t gwen_conv3x3_pack_bytes(int64_t Cin, int64_t Cout, int contract);
int gwen_conv3x3_pack_f32(const float *W, int64_t Cin, int64_t Cout, int transposed, int contract, void *packed,
                          gwen_stream_t stream);
int gwen_conv3x3_plan(int64_t H, int64_t W, int64_t Cin, int64_t Cout, int flags, int *column_tiles, int *slices);
int64_t gwen_conv3x3_workspace_floats(int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int flags);
int gwen_conv3x3_f32(const float *x, const void *packed, const float *bias, const float *scale, const float *shift,
                     float *out, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t ldx, int64_t ldo,
                     int flags, int contract, float *workspace, int64_t workspace_floats, gwen_stream_t stream);
int gwen_upsample2x_f32(const float *x, const float *scale, const float *shift, float *out, int64_t B, int64_t Hin,
                        int64_t Win, int64_t C, int64_t ldx, int64_t ldo, int flags, gwen_stream_t stream);
int64_t gwen_channel_stats_workspace_bytes(int64_t rows, int64_t C);
int gwen_channel_stats_f64(const float *x, int64_t rows, int64_t C, int64_t ld, double *mean, double *var,
                           void *workspace, int64_t workspace_bytes, gwen_stream_t stream);
int gwen_affine_relu_f32(float *x, const float *scale, const float *shift, int64_t rows, int64_t C, int64_t ld,
                         gwen_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * U-Net backward (csrc/conv.hip, csrc/conv_bwd.hip; gwen_amd.models_cnn with grad=True).  Same conventions as above:
 * channels-last fp32 rows with a pitch, no atomics, a fixed summation order (bitwise reproducible), 64-bit element
 * offsets, no host synchronisation, tensors of 4 GiB or more GWEN_ERANGE, bad arguments GWEN_EINVAL before any HIP call.
 * The data gradient of a 3x3 convolution is gwen_conv3x3_f32 with the weight packed as the OTHER layer type.
 *
 *   gwen_conv3x3_argmax_f32: gwen_conv3x3_f32 (same plan, same accumulation, the same bits in out) that also keeps
 *         what the backward needs of the pool.  Only legal with GWEN_CONV_POOL (else GWEN_EINVAL).  argmax (required):
 *         uint8 [B, H / 2, W / 2, Cout], packed -- the winner of the window in the order (0,0) (0,1) (1,0) (1,1): the
 *         first strictly largest value, a NaN replacing whatever came before it (torch's max_pool2d rule).  pre
 *         (optional, pitch ldp >= Cout): the pooled value + bias before the affine and the ReLU.
 *   gwen_conv3x3_grad_weight_f32: gw[co][ci][ky][kx] = sum_{b, y, x} g[b, y, x, co] x[b, y + ky - 1, x + kx - 1, ci]
 *         (zeros outside the image), g [B, H, W, Cout] pitch ldg, x [B, H, W, Cin] pitch ldx, gw a Conv2d's
 *         [Cout, Cin, 3, 3]; transposed = 1 writes a ConvTranspose2d's [Cin, Cout, 3, 3] with the taps flipped
 *         (Cin = the channels of x, the layer's input).  Split contractions only, both operands split on the fly.
 *         The pixel tiles of 8 x 16 are cut into chunks, each writing its raw sums once to a slab of workspace
 *         ([chunks][9 Cin Cout] floats); the slabs are added in chunk order (gwen_reduce_chunks_batched).
 *         gwen_conv3x3_grad_weight_workspace_floats: the floats needed (0: one chunk, workspace may be NULL; -1: out
 *         of range -- the slabs or an input would reach 4 GiB -- and the launcher answers GWEN_ERANGE; shorter:
 *         GWEN_ENOSPACE).  gwen_conv3x3_grad_weight_plan reports the cut: channel tiles of 16 x 16 per block (1, 2
 *         or 4) and pixel chunks.  The launcher and the size function read the same plan; the cut is a function of
 *         the shapes only.  An empty batch or image writes zeros.
 *   gwen_upsample2x_backward_f32: out [B, Hin, Win, C] = the adjoint of gwen_upsample2x_f32 applied to g
 *         [B, 2 Hin, 2 Win, C]: every input pixel sums the output pixels that read it in ascending (oy, ox), with the
 *         forward's own weights.  mask (optional, the shape of g, pitch ldm): g counts only where mask > 0.
 *   gwen_norm_relu_backward_f32: y = relu(gamma xhat + beta), xhat = (pre - mean) rstd, over rows x C.  g_z = g_y
 *         [y > 0]; sums[0][c] = g_beta = sum g_z and sums[1][c] = g_gamma = sum g_z xhat in fp64 (two stages in a fixed
 *         order, as gwen_channel_stats_f64; workspace of gwen_channel_stats_workspace_bytes(rows, C) bytes);
 *         g_pre = gamma rstd (g_z - g_beta / rows - xhat g_gamma / rows) (train = 1, mean and rstd the batch's) or
 *         gamma rstd g_z (train = 0, the running statistics) in fp32.  g_pre overlaps no input.
 *   gwen_unpool2x2_f32: out [B, H, W, C] = g_p [B, H / 2, W / 2, C] at each window's argmax, zeros elsewhere (the
 *         last odd row / column included).
 * ------------------------------------------------------------------------------------------- */
int gwen_conv3x3_argmax_f32(const float *x, const void *packed, const float *bias, const float *scale,
                            const float *shift, float *out, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                            int64_t ldx, int64_t ldo, int flags, int contract, float *workspace,
                            int64_t workspace_floats, uint8_t *argmax, float *pre, int64_t ldp, gwen_stream_t stream);
int gwen_conv3x3_grad_weight_plan(int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int *channel_tiles,
                                  int64_t *pixel_chunks);
int64_t gwen_conv3x3_grad_weight_workspace_floats(int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout);
int gwen_conv3x3_grad_weight_f32(const float *g, const float *x, float *gw, int64_t B, int64_t H, int64_t W,
                                 int64_t Cin, int64_t Cout, int64_t ldg, int64_t ldx, int transposed, int contract,
                                 float *workspace, int64_t workspace_floats, gwen_stream_t stream);
int gwen_upsample2x_backward_f32(const float *g, const float *mask, float *out, int64_t B, int64_t Hin, int64_t Win,
                                 int64_t C, int64_t ldg, int64_t ldm, int64_t ldo, gwen_stream_t stream);
int gwen_norm_relu_backward_f32(const float *g_y, const float *y, const float *pre, const float *weight,
                                const double *mean, const double *rstd, float *g_pre, double *sums, int64_t rows,
                                int64_t C, int64_t ldg, int64_t ldy, int64_t ldp, int64_t ldo, int train,
                                void *workspace, int64_t workspace_bytes, gwen_stream_t stream);
int gwen_unpool2x2_f32(const float *g_p, const uint8_t *argmax, float *out, int64_t B, int64_t H, int64_t W, int64_t C,
                       int64_t ldg, int64_t ldo, gwen_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GWEN_HIP_H */
