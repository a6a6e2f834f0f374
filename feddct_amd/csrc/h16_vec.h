// h16_vec.h — the device code the 16-bit vector tiles share: the reduce
// (fedagg_h16.hip tile_vec16) and the chain segments over 16-bit buckets
// (fedagg_chain16.hip) walk the clients with the same loop and finish with
// the same stores, so that a chained reduction gives the one launch's bits by
// construction.  Everything here is inlined into the including unit's kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "conv16.h"
#include "reduce_impl.h"

namespace fa_h16 {
using namespace fa_k;

typedef __attribute__((address_space(1))) const u4 gcu4;

// (widen, widen2, narrow, narrow2, widen8, narrow8: conv16.h, shared with
// prox_h16.hip)

// 16-B non-temporal load of vector `vidx` (8 elements) past a uniform base.
__device__ __forceinline__ u4 ldu4(const uint16_t* base, uint32_t vidx) {
  return __builtin_nontemporal_load((gcu4*)base + vidx);
}
// The result store: a buffer store with the sc1 policy bit, the fp32
// reduce's (reduce_impl.h st_out: the broadcast reads the result next).
__device__ __forceinline__ void st_sc1(uint16_t* base, uint32_t vidx, u4 v) {
  const __amdgpu_buffer_rsrc_t r =
      __builtin_amdgcn_make_buffer_rsrc(base, (short)0, 0x7fffffff, 0x00020000);
  __builtin_amdgcn_raw_buffer_store_b128(v, r, (int)(16 * vidx), 0, 16);
}
// The wide result store (an fp32 result bucket): one 16-B store of fp32 at
// byte offset `off` past a uniform base, the same policy.
__device__ __forceinline__ void st_sc1_f4(float* base, uint32_t off, f4 v) {
  const __amdgpu_buffer_rsrc_t r =
      __builtin_amdgcn_make_buffer_rsrc(base, (short)0, 0x7fffffff, 0x00020000);
  __builtin_amdgcn_raw_buffer_store_b128(v, r, (int)off, 0, 16);
}
__device__ __forceinline__ f4 shfl4(f4 v, int src) {
  return f4{__shfl(v.x, src, 64), __shfl(v.y, src, 64), __shfl(v.z, src, 64),
            __shfl(v.w, src, 64)};
}

// Client i's bucket and weight through scalar loads only: the kernarg arrays
// (n <= kInline) or the device table through the constant address space.
template <bool TAB>
__device__ __forceinline__ const uint16_t* cptr16(KArgs& a, int i) {
  if constexpr (TAB) return (const uint16_t*)((const FA_CONST f32p*)a.tab32)[i];
  else return (const uint16_t*)a.c32[i];
}
template <bool TAB>
__device__ __forceinline__ float cw16(KArgs& a, int i) {
  if constexpr (TAB) return ((const FA_CONST float*)a.tabw)[i];
  else return a.w[i];
}

// The clients in slot order, the next client's loads issued before the
// current client's adds.  Lane vector u holds columns 8 * vi[u] .. + 7 in
// accumulators 2u (first four) and 2u + 1.  The n clients are rows row0 ..
// row0 + n - 1 of the whole reduction (0 in a plain reduce): the promotions
// fall where that row count says, with lp the whole reduction's level step.
template <int EL, int U, bool FULL, bool W, bool TAB>
__device__ __forceinline__ void clients16(KArgs& a, Acc<2 * U, true>& A, int n, int64_t start,
                                          const uint32_t (&vi)[U], const bool (&ok)[U], int lp,
                                          int mask, int row0) {
  const u4 zero = u4{0u, 0u, 0u, 0u};
  u4 cur[U], nxt[U];
  {
    const uint16_t* p = cptr16<TAB>(a, 0) + start;
#pragma unroll
    for (int u = 0; u < U; ++u) cur[u] = (FULL || ok[u]) ? ldu4(p, vi[u]) : zero;
  }
  for (int b = 0; b < n; ++b) {
    if (b + 1 < n) {
      const uint16_t* p = cptr16<TAB>(a, b + 1) + start;
#pragma unroll
      for (int u = 0; u < U; ++u) nxt[u] = (FULL || ok[u]) ? ldu4(p, vi[u]) : zero;
    }
    float wb = 0.f;
    if constexpr (W) wb = cw16<TAB>(a, b);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      f4 x0, x1;
      widen8<EL>(cur[u], &x0, &x1);
      if constexpr (W) {
        x0 = mul4s(x0, wb);
        x1 = mul4s(x1, wb);
      }
      A.l0[2 * u] = add4(A.l0[2 * u], x0);
      A.l0[2 * u + 1] = add4(A.l0[2 * u + 1], x1);
    }
    promote<2 * U, true>(A, row0 + b + 1, lp, mask);
#pragma unroll
    for (int u = 0; u < U; ++u) cur[u] = nxt[u];
  }
}

// The finish of a vector tile: l0 + l1, + l2, + l3, then / fn unless
// `sum_only`, rounded to nearest-even into the 16-bit bucket (WIDE: the fp32
// value unrounded into the fp32 bucket at the same element offsets) —
// fedagg_h16.hip tile_vec16's finish, statement for statement, for the chain
// segments' last launch.  tile_vec16 keeps its own inline text: calling this
// from it (tried with the accumulators by reference and by value, the sum
// flag as an argument and as a template parameter, and split into sums and
// stores) compiled every h16_round_kernel differently (64 more register
// moves in the 2048-element kernels), and that unit's code object stays
// byte-identical to the measured one.
template <int EL, int U, bool FULL, bool WIDE>
__device__ __forceinline__ void finish16(KArgs& a, const Acc<2 * U, true>& A, int64_t start,
                                         int count, const uint32_t (&vi)[U], const bool (&ok)[U],
                                         bool sum_only, float fn) {
  if constexpr (WIDE) {
    // A lane's 8 fp32 results are 32 B; stored from the lane that summed
    // them, as two adjacent 16-B stores, each store instruction covers only
    // every other 16 B of the wave's 2 KB, and the launch ran 11-12 us behind
    // the 16-bit one at N = 20 / 24 and 19 us at N = 5.  So the
    // wave first exchanges: for store s, lane t takes half t & 1 of lane
    // 32 s + t / 2, and each store instruction writes 1 KB contiguous, as the
    // 16-bit result store does.  Every lane takes part (one past the tile's
    // end holds +0 sums); a store goes out when its SOURCE lane is inside.
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      f4 r[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        f4 s = add4(A.l0[2 * u + h], A.l1[2 * u + h]);
        s = add4(s, A.l2[2 * u + h]);
        s = add4(s, A.l3[2 * u + h]);
        r[h] = sum_only ? s : div4s(s, fn);
      }
      const uint32_t wv0 = vi[u] - lane;  // the wave's first vector
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const uint32_t src = 32 * s + (lane >> 1);
        const f4 lo = shfl4(r[0], (int)src), hi = shfl4(r[1], (int)src);
        const f4 v = (lane & 1) ? hi : lo;
        if (FULL || (int)(kVec * (wv0 + src)) < count)
          st_sc1_f4(a.out32 + start, 32 * wv0 + 1024 * s + 16 * lane, v);
      }
    }
    return;
  }
  uint16_t* out = (uint16_t*)a.out32 + start;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (!ok[u]) continue;
    f4 r[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f4 s = add4(A.l0[2 * u + h], A.l1[2 * u + h]);
      s = add4(s, A.l2[2 * u + h]);
      s = add4(s, A.l3[2 * u + h]);
      r[h] = sum_only ? s : div4s(s, fn);
    }
    st_sc1(out, vi[u],
           u4{narrow2<EL>(r[0].x, r[0].y), narrow2<EL>(r[0].z, r[0].w),
              narrow2<EL>(r[1].x, r[1].y), narrow2<EL>(r[1].z, r[1].w)});
  }
}

}  // namespace fa_h16
