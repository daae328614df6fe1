// Phase 1 of K4 / K5: gather + aggregate destination rows from the GROUPED layout (gwen_gcn_group8).
//
// One wave handles R = 64 / (FIN/4) rows per pass (FIN/4 lanes per row, 16-B loads) and NP passes.
// Every load is unconditional (absent rows read the all-zero null group): a load under a per-lane
// condition makes hipcc branch around it and wait vmcnt(0), which serialises the gathers.
// The passes are software-pipelined by hand -- the compiler keeps them strictly one after another:
// the column indices of pass p+1 are requested before pass p's row gathers are waited for, and
// pass p's weights ride along with its gathers, so a pass costs one memory round trip, not two.
// UNI: uniform layout (every row exactly one group, rowptr == NULL): row r is the group at 8 r.
// GE: entries of a group that are gathered (8, or 7 on a uniform layout whose rows all hold at most 7
// entries -- a geodesic mesh: 6 neighbours + the self loop -- so that slot 7 is padding on EVERY row).
// With GE = 7 the slot's row load and its 4 FMAs are not issued; the two 16-B index loads and the two
// 16-B weight loads stay whole and the layout is the same.  It is a template argument, never a per-lane
// or per-row branch, for the reason above: every load that is issued stays unconditional.
// Results: the skipped term is fma(0, v, acc), so for finite inputs every value is the same; only the
// sign of an exact zero can differ (-0 + 0 = +0), and an Inf / NaN in the row of a destination's FIRST
// entry (the pad slot's column) no longer turns the sum into NaN through 0 * Inf.
// D: gather depth, the passes of row loads a wave keeps in flight (1 or 2).  D = 1 is the loop above: a wave has
// at most GE loads outstanding and runs a pass's FMAs / split / LDS writes with nothing behind them.  D = 2 issues
// the row loads of pass p+1 BEFORE pass p's FMAs, into a second register buffer (two buffers, alternated by hand in
// a loop over PAIRS of passes that stays rolled; the last two or three passes are peeled), and requests the column indices
// two passes ahead -- before the row loads of the pass in between, because vmcnt retires in issue order: indices
// requested after those row loads could only be waited for together with them.  Issue order per pass q:
//   indices(q+2)  <  rows + weights(q+1)  <  FMAs, sink(q)
// so the wait for rows(q) leaves indices(q+2) and rows(q+1) outstanding.  Arithmetic is D = 1's, term for term:
// every value is bitwise the same.  On the non-uniform layout `locate` itself loads (row pointers, then indices),
// and its wait drains the older row loads: D = 2 is correct there but only overlaps the vector work.
// shadow(): a second callable, run exactly ONCE, after the row loads of the FIRST pass have been issued and before
// their first wait (D = 1: between the loads and the FMAs of pass 0; D = 2: after request(0), request(1), issue(A)).
// It is where K4 / K5 split W into bf16 images: the raw W loads are issued at the top of the kernel, before the first
// index request and with no wait in between; vmcnt retires in issue order, so they have landed when the first indices
// have, and the split's vector work runs while the first rows are in flight instead of in front of the whole chain.
// The order is pinned with sched_barrier.  With a shadow the depth-1 loop has its first pass peeled (the callable
// must not sit under a condition inside the rolled loop); NoShadow keeps the loop exactly as it was -- the persistent
// wide kernels and the backward compile to the code they had.
// IM: how a pass's indices and weights reach its lanes (index mode).  1: every lane of the FIN/4 that share a destination
// row loads the row's whole group itself -- 32 B of col and 32 B of val, four 16-B loads per lane and pass for 64 unique
// bytes per row.  2 (uniform layout only): the "record" form.  The row's record is [col[s .. s+7] | val[s .. s+7]]; lane
// gl of the row's G = FIN/4 lanes loads only its 64/G-byte share of it with ONE load per pass (dword / dwordx2 /
// dwordx4 at G = 16 / 8 / 4; the lower half of the lanes from col + s, the upper half from val + s: the base pointer is
// selected per lane, the load stays unconditional, absent rows read the null group), and the indices and weights are
// broadcast inside the lane group without memory (group_bcast).  The weights are broadcast at consume time from the
// kept record, so a pass in flight holds the record (1, 2 or 4 registers), not 8 registers of weights.  Issue order,
// vmcnt order, the shadow's place and the arithmetic -- the same fma chain over the slots in slot order -- are those of
// IM = 1 with "record" for "indices": every value is bitwise the same.  IM = 1 compiles to the code it had.
#pragma once
#include <type_traits>
#include <utility>

#include "common.h"

namespace gwen {

typedef int int4_u __attribute__((ext_vector_type(4), aligned(4)));
typedef float float4_u __attribute__((ext_vector_type(4), aligned(4)));

template <int FIN, int GE = 8>
__device__ inline float4_t gather_group(const char *xb, uint32_t lane_off, const int4_u &c0,
                                        const int4_u &c1, const float4_u &w0, const float4_u &w1,
                                        float4_t acc) {
  constexpr uint32_t kRowBytes = FIN * 4;        // x rows are contiguous: base + 32-bit byte offset
  static_assert(GE == 7 || GE == 8, "a group is gathered whole or without its last slot");
  float4_t v[GE];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    v[u] = *reinterpret_cast<const float4_t *>(xb + (uint64_t)((uint32_t)c0[u] * kRowBytes + lane_off));
    if (u + 4 < GE)
      v[u + 4] = *reinterpret_cast<const float4_t *>(xb + (uint64_t)((uint32_t)c1[u] * kRowBytes + lane_off));
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
    acc = __builtin_elementwise_fma(float4_t{w0[u], w0[u], w0[u], w0[u]}, v[u], acc);
#pragma unroll
  for (int u = 0; u < GE - 4; ++u)
    acc = __builtin_elementwise_fma(float4_t{w1[u], w1[u], w1[u], w1[u]}, v[u + 4], acc);
  return acc;
}

// gather_group in two halves (D = 2): the row loads of one group, and -- later -- its FMAs in the same slot order
// KEEP: see the end of the body; asked for where further index loads are in flight behind this group's
template <int FIN, int GE, bool KEEP>
__device__ __forceinline__ void issue_group(const char *xb, uint32_t lane_off, const int4_u &c0, const int4_u &c1,
                                            float4_t (&v)[GE]) {
  constexpr uint32_t kRowBytes = FIN * 4;
  static_assert(GE == 7 || GE == 8, "a group is gathered whole or without its last slot");
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    v[u] = *reinterpret_cast<const float4_t *>(xb + (uint64_t)((uint32_t)c0[u] * kRowBytes + lane_off));
    if (u + 4 < GE)
      v[u + 4] = *reinterpret_cast<const float4_t *>(xb + (uint64_t)((uint32_t)c1[u] * kRowBytes + lane_off));
  }
  // GE = 7: c1[3] is never read, and the register allocator hands its register out again while the 16-B index load
  // that writes it is still in flight -- the overwrite then waits vmcnt(0) for that load, the youngest one, and
  // with it for every row load in front of it.  A (free) use of the whole vector behind the row addresses keeps
  // the register taken until the indices have been waited for anyway.  It costs registers (K4 16 -> 32: 57 -> 62, a wave),
  // so it is only asked for where a younger index request exists: every depth-2 pass, and depth 1 with NP > 1.
  if constexpr (GE == 7 && KEEP) asm volatile("" ::"v"(c1));
}

template <int GE>
__device__ __forceinline__ float4_t fma_group(const float4_t (&v)[GE], const float4_u &w0, const float4_u &w1,
                                              float4_t acc) {
#pragma unroll
  for (int u = 0; u < 4; ++u)
    acc = __builtin_elementwise_fma(float4_t{w0[u], w0[u], w0[u], w0[u]}, v[u], acc);
#pragma unroll
  for (int u = 0; u < GE - 4; ++u)
    acc = __builtin_elementwise_fma(float4_t{w1[u], w1[u], w1[u], w1[u]}, v[u + 4], acc);
  return acc;
}

// one register buffer of the depth-2 gather: a pass's indices (c, s, rb: requested), then its rows and weights
// (v, w; is, irb: the group offset and row end of the pass whose rows are in v)
template <int GE>
struct GatherBuf {
  int4_u c0, c1;
  int32_t s, rb, is, irb;
  float4_u w0, w1;
  float4_t v[GE];
};

// v where keep, else +0 in every lane: the unconditional form of `if (p) v = *p` (load from an address that is always
// valid, then mask).  Written as a mask because the optimiser sinks a load whose only use is conditional back under
// the condition -- and a load under a condition is what the rule above forbids.
__device__ __forceinline__ float4_t masked_f4(float4_t v, bool keep) {
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  const uint32_t m = keep ? 0xffffffffu : 0u;
  return __builtin_bit_cast(float4_t, __builtin_bit_cast(u4, v) & u4{m, m, m, m});
}

// The record form (IM = 2): a lane's share of its row's record, DW = 16 / G dwords
typedef uint32_t uint2_u __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t uint4_u __attribute__((ext_vector_type(4), aligned(4)));
template <int DW> struct Record;
template <> struct Record<1> {
  using T = uint32_t;
  static __device__ __forceinline__ uint32_t get(const T &r, int) { return r; }
};
template <> struct Record<2> {
  using T = uint2_u;
  static __device__ __forceinline__ uint32_t get(const T &r, int i) { return r[i]; }
};
template <> struct Record<4> {
  using T = uint4_u;
  static __device__ __forceinline__ uint32_t get(const T &r, int i) { return r[i]; }
};

// v of lane SRC of this lane's group of G consecutive lanes (G = 4, 8, 16: inside the 32 lanes of a swizzle), in
// every lane of the group: ds_swizzle in bit-mask mode, lane' = (lane & ~(G - 1)) | SRC.  No LDS memory is touched.
template <int G, int SRC>
__device__ __forceinline__ uint32_t group_bcast(uint32_t v) {
  static_assert((G == 4 || G == 8 || G == 16) && SRC >= 0 && SRC < G, "a lane group inside a swizzle group");
  return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (~(G - 1) & 31) | (SRC << 5));
}

// slots 0 .. GE-1 of one half of the record (FIRST = 0: the column indices, G / 2: the weights), broadcast to the group
template <int G, int FIRST, int... U>
__device__ __forceinline__ void record_slots(const typename Record<16 / G>::T &rec, uint32_t (&o)[sizeof...(U)],
                                             std::integer_sequence<int, U...>) {
  constexpr int DW = 16 / G;
  ((o[U] = group_bcast<G, FIRST + U / DW>(Record<DW>::get(rec, U % DW))), ...);
}

// the row loads of a pass from its record, and -- later -- its FMAs with the weights of the kept record: issue_group and
// fma_group of the record form, slot for slot
template <int FIN, int GE>
__device__ __forceinline__ void issue_record(const char *xb, uint32_t lane_off,
                                             const typename Record<64 / FIN>::T &rec, float4_t (&v)[GE]) {
  constexpr uint32_t kRowBytes = FIN * 4;
  static_assert(GE == 7 || GE == 8, "a group is gathered whole or without its last slot");
  uint32_t c[GE];
  record_slots<FIN / 4, 0>(rec, c, std::make_integer_sequence<int, GE>{});
#pragma unroll
  for (int u = 0; u < 4; ++u) {                            // issue_group's order of slots: 0, 4, 1, 5, ...
    v[u] = *reinterpret_cast<const float4_t *>(xb + (uint64_t)(c[u] * kRowBytes + lane_off));
    if (u + 4 < GE)
      v[u + 4] = *reinterpret_cast<const float4_t *>(xb + (uint64_t)(c[u + 4] * kRowBytes + lane_off));
  }
}

template <int FIN, int GE>
__device__ __forceinline__ float4_t fma_record(const float4_t (&v)[GE], const typename Record<64 / FIN>::T &rec,
                                               float4_t acc) {
  uint32_t wb[GE];
  record_slots<FIN / 4, FIN / 8>(rec, wb, std::make_integer_sequence<int, GE>{});
#pragma unroll
  for (int u = 0; u < GE; ++u) {
    const float w = __builtin_bit_cast(float, wb[u]);
    acc = __builtin_elementwise_fma(float4_t{w, w, w, w}, v[u], acc);
  }
  return acc;
}

struct NoShadow {
  __device__ __forceinline__ void operator()() const {}
};

// sink(lr, acc): lr = row index inside the block (p * RB + wave * R + gr), acc = aggregated 4 floats
template <int FIN, int NP, int RB, bool UNI, int GE = 8, int D = 1, int IM = 1, typename Sink,
          typename Shadow = NoShadow>
__device__ inline void gather_passes(const int32_t *__restrict__ rowptr,
                                     const int32_t *__restrict__ col,
                                     const float *__restrict__ val, const char *xb, int32_t N,
                                     int b0, int wave, int gr, uint32_t lane_off, Sink &&sink,
                                     Shadow &&shadow = Shadow{}) {
  constexpr int R = 64 / (FIN / 4);
  constexpr bool kShadow = !std::is_same<std::decay_t<Shadow>, NoShadow>::value;
  static_assert(GE == 8 || UNI, "only the uniform layout bounds a row by one group");
  // group offset and row end of pass p (absent rows: the null group, which ends at once)
  auto locate = [&](int p, int32_t &s, int32_t &rb) {
    const int r = b0 + p * RB + wave * R + gr;
    const bool ok = r < N;
    if constexpr (UNI) {
      s = ok ? 8 * r : 8 * N;
      rb = 0;
    } else {
      const int32_t ra = rowptr[ok ? r : N];
      rb = rowptr[ok ? r + 1 : N];
      s = rb > ra ? ra : rowptr[N];
    }
  };
  static_assert(D == 1 || D == 2, "one or two passes of row loads in flight");
  static_assert(IM == 1 || (IM == 2 && UNI && FIN <= 64), "the record form: uniform layout, up to 64 channels");
  if constexpr (IM == 2) {
    constexpr int G = FIN / 4, DW = 16 / G;
    using Rec = typename Record<DW>::T;
    // this lane's share of the record of pass p: lanes 0 .. G/2-1 of the row read col + s, the others val + s
    const uint32_t gl = lane_off / 16;
    const char *half = (gl < G / 2 ? reinterpret_cast<const char *>(col) : reinterpret_cast<const char *>(val)) +
                       (gl % (G / 2)) * (4 * DW);
    auto request = [&](int p) {
      int32_t s, rb;
      locate(p, s, rb);
      const Rec r = *reinterpret_cast<const Rec *>(half + (int64_t)s * 4);
      __builtin_amdgcn_sched_barrier(0);
      return r;
    };
    if constexpr (D == 2 && NP > 1) {
      struct Buf {
        Rec rec, irec;                                     // requested; of the pass whose rows are in v
        float4_t v[GE];
      };
      auto issue = [&](Buf &b) {
        b.irec = b.rec;
        issue_record<FIN, GE>(xb, lane_off, b.rec, b.v);
        __builtin_amdgcn_sched_barrier(0);
      };
      auto consume = [&](int p, const Buf &b) {
        sink(p * RB + wave * R + gr, fma_record<FIN, GE>(b.v, b.irec, float4_t{0.f, 0.f, 0.f, 0.f}));
        __builtin_amdgcn_sched_barrier(0);
      };
      Buf A, B;                                            // the loop of IM = 1 below, step for step
      A.rec = request(0);
      B.rec = request(1);
      issue(A);
      if constexpr (kShadow) {
        shadow();
        __builtin_amdgcn_sched_barrier(0);
      }
      auto step = [&](int q, Buf &X, Buf &Y) {
        X.rec = request(q + 2);
        issue(Y);
        consume(q, X);
      };
#pragma unroll 1
      for (int p = 0; p + 3 < NP; p += 2) {
        step(p, A, B);
        step(p + 1, B, A);
      }
      if constexpr (NP % 2 == 1) {
        step(NP - 3, A, B);
        issue(A);
        consume(NP - 2, B);
        consume(NP - 1, A);
      } else {
        issue(B);
        consume(NP - 2, A);
        consume(NP - 1, B);
      }
    } else {
      // depth 1: the next pass's record is requested before this pass's row loads are waited for
      Rec rec = request(0);
      auto pass = [&](int p, bool more, auto &&between) {
        Rec nrec = rec;
        if (more) nrec = request(p + 1);
        float4_t v[GE];
        issue_record<FIN, GE>(xb, lane_off, rec, v);
        __builtin_amdgcn_sched_barrier(0);
        between();
        sink(p * RB + wave * R + gr, fma_record<FIN, GE>(v, rec, float4_t{0.f, 0.f, 0.f, 0.f}));
        rec = nrec;
      };
      if constexpr (kShadow) {
        pass(0, NP > 1, [&]() {
          shadow();
          __builtin_amdgcn_sched_barrier(0);
        });
      }
#pragma unroll 1
      for (int p = kShadow ? 1 : 0; p < NP; ++p) pass(p, p + 1 < NP, []() {});
    }
    return;
  }
  if constexpr (D == 2 && NP > 1) {
    using Buf = GatherBuf<GE>;
    auto request = [&](int p, Buf &b) {                    // indices of pass p
      locate(p, b.s, b.rb);
      b.c0 = *reinterpret_cast<const int4_u *>(col + b.s);
      b.c1 = *reinterpret_cast<const int4_u *>(col + b.s + 4);
      __builtin_amdgcn_sched_barrier(0);                   // the issue order above is the point: pin it
    };
    auto issue = [&](Buf &b) {                             // rows and weights of the pass whose indices b holds
      b.is = b.s; b.irb = b.rb;
      b.w0 = *reinterpret_cast<const float4_u *>(val + b.s);
      b.w1 = *reinterpret_cast<const float4_u *>(val + b.s + 4);
      issue_group<FIN, GE, true>(xb, lane_off, b.c0, b.c1, b.v);
      __builtin_amdgcn_sched_barrier(0);
    };
    auto consume = [&](int p, const Buf &b) {
      float4_t acc = fma_group<GE>(b.v, b.w0, b.w1, float4_t{0.f, 0.f, 0.f, 0.f});
      if constexpr (!UNI) {
        for (int32_t q = b.is + 8; q < b.irb; q += 8) {    // rows longer than one group: finished here, in order
          const int4_u d0 = *reinterpret_cast<const int4_u *>(col + q);
          const int4_u d1 = *reinterpret_cast<const int4_u *>(col + q + 4);
          const float4_u x0 = *reinterpret_cast<const float4_u *>(val + q);
          const float4_u x1 = *reinterpret_cast<const float4_u *>(val + q + 4);
          acc = gather_group<FIN>(xb, lane_off, d0, d1, x0, x1, acc);
        }
      }
      sink(p * RB + wave * R + gr, acc);
      __builtin_amdgcn_sched_barrier(0);
    };
    Buf A, B;
    request(0, A);
    request(1, B);
    issue(A);
    if constexpr (kShadow) {
      shadow();
      __builtin_amdgcn_sched_barrier(0);
    }
    // One step in the steady state: X holds the rows of pass q (in flight), Y the indices of pass q+1.
    auto step = [&](int q, Buf &X, Buf &Y) {
      request(q + 2, X);
      issue(Y);
      consume(q, X);
    };
    // Rolled over PAIRS of steps, the two buffers written out by hand: hipcc can not hoist a third pass.  Every
    // step of the loop issues the same loads, and the last two passes are peeled, so that each wait has ONE count of
    // loads behind it -- a consume shared by a path that issued the next pass and one that did not waits vmcnt(0).
#pragma unroll 1
    for (int p = 0; p + 3 < NP; p += 2) {
      step(p, A, B);
      step(p + 1, B, A);
    }
    if constexpr (NP % 2 == 1) {
      step(NP - 3, A, B);
      issue(A);
      consume(NP - 2, B);
      consume(NP - 1, A);
    } else {
      issue(B);
      consume(NP - 2, A);
      consume(NP - 1, B);
    }
    return;
  }
  int32_t s, rb;
  locate(0, s, rb);
  int4_u c0 = *reinterpret_cast<const int4_u *>(col + s);
  int4_u c1 = *reinterpret_cast<const int4_u *>(col + s + 4);
  if constexpr (kShadow) {
    // pass 0 written out, in the loop's own order, with the shadow between its row loads and its FMAs
    int4_u n0 = c0, n1 = c1;
    int32_t ns = s, nrb = rb;
    if constexpr (NP > 1) {
      locate(1, ns, nrb);
      n0 = *reinterpret_cast<const int4_u *>(col + ns);
      n1 = *reinterpret_cast<const int4_u *>(col + ns + 4);
    }
    const float4_u w0 = *reinterpret_cast<const float4_u *>(val + s);
    const float4_u w1 = *reinterpret_cast<const float4_u *>(val + s + 4);
    float4_t v[GE];
    issue_group<FIN, GE, (NP > 1)>(xb, lane_off, c0, c1, v);
    __builtin_amdgcn_sched_barrier(0);
    shadow();
    __builtin_amdgcn_sched_barrier(0);
    float4_t acc = fma_group<GE>(v, w0, w1, float4_t{0.f, 0.f, 0.f, 0.f});
    if constexpr (!UNI) {
      for (int32_t q = s + 8; q < rb; q += 8) {
        const int4_u d0 = *reinterpret_cast<const int4_u *>(col + q);
        const int4_u d1 = *reinterpret_cast<const int4_u *>(col + q + 4);
        const float4_u x0 = *reinterpret_cast<const float4_u *>(val + q);
        const float4_u x1 = *reinterpret_cast<const float4_u *>(val + q + 4);
        acc = gather_group<FIN>(xb, lane_off, d0, d1, x0, x1, acc);
      }
    }
    sink(wave * R + gr, acc);
    c0 = n0; c1 = n1; s = ns; rb = nrb;
  }
  // a rolled loop: fully unrolled, hipcc hoists several passes' gathers at once and the register
  // count (172 VGPRs at Fin = 128) costs more occupancy than the extra overlap returns
#pragma unroll 1
  for (int p = kShadow ? 1 : 0; p < NP; ++p) {
    int4_u n0 = c0, n1 = c1;
    int32_t ns = s, nrb = rb;
    if (p + 1 < NP) {                                    // next pass's source rows, one pass ahead
      locate(p + 1, ns, nrb);
      n0 = *reinterpret_cast<const int4_u *>(col + ns);
      n1 = *reinterpret_cast<const int4_u *>(col + ns + 4);
    }
    const float4_u w0 = *reinterpret_cast<const float4_u *>(val + s);
    const float4_u w1 = *reinterpret_cast<const float4_u *>(val + s + 4);
    float4_t acc = gather_group<FIN, GE>(xb, lane_off, c0, c1, w0, w1, float4_t{0.f, 0.f, 0.f, 0.f});
    if constexpr (!UNI) {
      for (int32_t q = s + 8; q < rb; q += 8) {          // rows longer than one group of 8
        const int4_u d0 = *reinterpret_cast<const int4_u *>(col + q);
        const int4_u d1 = *reinterpret_cast<const int4_u *>(col + q + 4);
        const float4_u x0 = *reinterpret_cast<const float4_u *>(val + q);
        const float4_u x1 = *reinterpret_cast<const float4_u *>(val + q + 4);
        acc = gather_group<FIN>(xb, lane_off, d0, d1, x0, x1, acc);
      }
    }
    sink(p * RB + wave * R + gr, acc);
    c0 = n0; c1 = n1; s = ns; rb = nrb;
  }
}

// The 16-byte output store of K4 / K5's epilogues and of k_gather.  ST (the kernels' store mode):
//   1  a plain store -- the statement the kernels had, instruction for instruction;
//   3  the same address and bytes WRITTEN THROUGH (the sc1 bit): the line goes to memory at the store and leaves the XCD's
//      L2, so the launch leaves nothing dirty behind for its boundary to write back.  No launch of a stack finds its input
//      in L2 anyway (profiles/xcd_pmc.tsv), so dropping the line costs the next launch nothing.  Visibility is unchanged: the
//      kernel boundary still releases.  hipcc does not count an asm store (nothing reads it back in the kernel, and a wave's
//      stores complete after it ends), and the trailing s_nop 1 keeps the data registers from being rewritten before the
//      store has read them.
// Modes 2 and 4 of the C ABI stay reserved numbers (refused).  Whole rows through an LDS out tile are not a store mode but
// a switch of their own beside it, k_layer's RS (layer.hip, "Row stores"): its row stores go through store_out<3>.
template <int ST>
__device__ __forceinline__ void store_out(float *p, float4_t v) {
  static_assert(ST == 1 || ST == 3, "store modes: 1 plain, 3 written through");
  if constexpr (ST == 3)
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
  else
    *reinterpret_cast<float4_t *>(p) = v;
}

}  // namespace gwen
