// What the kernels over an ensemble's members axis share (ensemble.hip, products.hip, refloss.hip, loss.hip): the member
// chains, the register bitonic network, the fixed-order block sum, and on the host the pass geometry, the member-bucket
// dispatch and the argument checks.  Each is written once, with the reason for its form beside it.
#pragma once
#include "common.h"
#include "dispatch.h"

#include <initializer_list>
#include <type_traits>
#include <utility>

namespace gwen::ens {

__device__ inline float sgnf(float d) { return d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f); }

// ---- member chains ------------------------------------------------------------------------------------------------------

// f(i) for the members i < M, i a compile-time index (registers): a chain of uniform branches that ends at M.  A
// predicate per member instead is if-converted into selects whose MB conditions the compiler computes up front and keeps
// in scalar registers (spilled from 16 members up), and a loop with a break at M is not fully unrolled past 8 (the
// member arrays then go to scratch).
template <int I, int MB, typename F>
__device__ __forceinline__ void members(int M, F &&f) {
  if constexpr (I < MB) {
    if (I >= M) return;
    f(std::integral_constant<int, I>());
    members<I + 1, MB>(M, f);
  }
}

// f(i) for i = MB - 1 down to M: the pads of a sorting network, set by a chain of their own.  Initialised in front of the
// loads, every exit of the load chain re-materialises all pads above it (MB^2 / 2 moves a point).
template <int I, typename F>
__device__ __forceinline__ void pads(int M, F &&f) {
  if constexpr (I >= 0) {
    if (I < M) return;
    f(std::integral_constant<int, I>());
    pads<I - 1>(M, f);
  }
}

// M through an empty asm in front of a chain: otherwise the MB conditions of the first chain are kept in scalar
// registers for the later ones, and spill from 32 members up
__device__ __forceinline__ int fresh(int m) {
  asm volatile("" : "+s"(m));
  return m;
}

// M and the plane stride through an empty asm once a node: otherwise the compiler hoists the MB member addresses (two
// scalar registers each) out of the node loop, and they spill from 8 members up.  The member address itself then passes
// an empty asm as a VECTOR register, "+v", in the kernel: no scalar base per member.
__device__ __forceinline__ void fresh(int &m, int64_t &plane) { asm volatile("" : "+s"(m), "+s"(plane)); }

// ---- register bitonic network ---------------------------------------------------------------------------------------------

// s[0 .. MB) ascending, MB a power of two, every index a compile-time one.  IDX: the member indices id[] travel with the
// values -- one compare whose lane mask feeds four selects at once; the scheduling barrier keeps the compiler from
// hoisting a stage's compares (a mask each, two scalar registers) ahead of their selects, which spills scalar registers
// at 32 and 64 members.  Values only (id unused): min / max, which drop a NaN silently.
__device__ inline void cex(float &a, float &b, int &ia, int &ib, bool up) {
  const bool sw = up ? (b < a) : (a < b);
  const float ta = a;
  a = sw ? b : a;
  b = sw ? ta : b;
  const int t = ia;
  ia = sw ? ib : ia;
  ib = sw ? t : ib;
  __builtin_amdgcn_sched_barrier(0);
}
__device__ inline void cex(float &a, float &b, bool up) {
  const float lo = __builtin_fminf(a, b), hi = __builtin_fmaxf(a, b);
  a = up ? lo : hi;
  b = up ? hi : lo;
}
template <int MB, bool IDX>
__device__ __forceinline__ void bitonic_sort(float *s, int *id = nullptr) {
#pragma unroll
  for (int k = 2; k <= MB; k <<= 1)
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1)
#pragma unroll
      for (int i = 0; i < MB; ++i) {
        const int l = i ^ j;
        if (l > i) {
          if constexpr (IDX) cex(s[i], s[l], id[i], id[l], (i & k) == 0);
          else cex(s[i], s[l], (i & k) == 0);
        }
      }
}

// ---- block sums -----------------------------------------------------------------------------------------------------------

// K sums over the block's THREADS threads at once, in a fixed order (a tree over LDS: bitwise reproducible, no atomics):
// red[k][0] = the sum of every thread's v[k], valid after the call.  red: K LDS rows of THREADS entries (&row for one).
// (The rows are a pack, Ks = 0 .. K - 1, not a loop: with a loop over k around them the compiler lays the unrolled tree
// out differently from the same tree written by hand.)
template <int THREADS, typename T, int... Ks>
__device__ __forceinline__ void block_sum_rows(T (*red)[THREADS], const T (&v)[sizeof...(Ks)],
                                               std::integer_sequence<int, Ks...>) {
  ((red[Ks][threadIdx.x] = v[Ks]), ...);
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) ((red[Ks][threadIdx.x] += red[Ks][threadIdx.x + s]), ...);
    __syncthreads();
  }
}
template <int THREADS, int K, typename T>
__device__ __forceinline__ void block_sum(T (*red)[THREADS], const T (&v)[K]) {
  block_sum_rows<THREADS>(red, v, std::make_integer_sequence<int, K>());
}

// one sum, returned to every thread; red is free for the next sum on return
template <int THREADS>
__device__ __forceinline__ float block_sum_all(float acc, float (*red)[THREADS]) {
  block_sum<THREADS>(red, {acc});
  const float r = red[0][0];
  __syncthreads();
  return r;
}

// ---- host: geometry, dispatch, checks -------------------------------------------------------------------------------------

// Thread (row, lc) of a block owns column bx * CT + lc and walks the nodes n = by * R + row, += gridDim.y * R: CT columns
// by R rows a block, gx blocks across the columns.  A function of the shapes alone.
struct ColumnTiles {
  int64_t CT, R, gx;
};
inline ColumnTiles column_tiles(int64_t cols, int64_t threads) {
  ColumnTiles t;
  t.CT = cols < threads ? cols : threads;
  t.R = threads / t.CT;
  t.gx = (cols + t.CT - 1) / t.CT;
  return t;
}

// The grid of a pass whose blocks walk the nodes: column_tiles of the C / VEC vector columns, and G node chunks -- as many
// as one resident set of blocks (no tail round), at most max_chunks.  `resident`, the blocks of THIS kernel instantiation
// the device holds at once, is asked once per instantiation and kept.
struct PassGeometry {
  int64_t CT, R, gx, G;
};
template <auto KERNEL, int THREADS>
int pass_geometry(int vec, int64_t C, int64_t N, int64_t max_chunks, PassGeometry &g) {
  static int resident = 0;
  if (resident == 0) {
    int dev = 0, cus = 0, per_cu = 0;
    GWEN_HIP_CHECK(hipGetDevice(&dev));
    GWEN_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    GWEN_HIP_CHECK(
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(KERNEL), THREADS, 0));
    resident = (cus < 8 ? 8 : cus) * (per_cu < 1 ? 1 : per_cu);
  }
  const ColumnTiles t = column_tiles(vec == 4 ? C / 4 : C, THREADS);
  int64_t cap = resident / t.gx;
  cap = cap < 1 ? 1 : (cap > max_chunks ? max_chunks : cap);
  const int64_t G = (N + t.R - 1) / t.R;
  g = PassGeometry{t.CT, t.R, t.gx, G < cap ? G : cap};
  return GWEN_OK;
}

// f(std::integral_constant<int, B>) for the member bucket of M: the first B of the list with M <= B, the last B when none
// has (0 in refloss.hip: any number of members, a run-time loop).  Returns what f returns.
template <int... Bs, class F>
int dispatch_bucket(gwen::ints<Bs...> buckets, int64_t M, F &&f) {
  constexpr int all[] = {Bs...};
  int64_t b = all[sizeof...(Bs) - 1];
  (void)((M <= Bs && ((b = Bs), true)) || ...);
  return gwen::dispatch(buckets, b, f);
}

// pred [M, N, C] as the CRPS, the products and the rank histogram address it: up to 64 members in registers, 4 C and the
// element count within the kernels' index types
inline bool shape_ok(int64_t M, int64_t N, int64_t C) {
  return M >= 1 && M <= 64 && N >= 1 && C >= 1 && C <= INT32_MAX / 4 && N <= (int64_t(1) << 40) / C;
}

// every pointer that is given is a-byte aligned
inline bool aligned_all(std::initializer_list<const void *> ptrs, size_t a) {
  for (const void *p : ptrs)
    if (p && !gwen_aligned(p, a)) return false;
  return true;
}

}  // namespace gwen::ens
