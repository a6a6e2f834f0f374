// fedagg_chain16.hip — chain segments of the cascade over fp16 / bf16 buckets
// (fa_reduce_chain_elem on an h16-family plan of vector tiles).  The clients
// are rows row0 .. row0 + n - 1 of an n_total-row reduction: the four level
// accumulators start from the fp32 state planes lev_in names (the others are
// +0 there), the clients are walked by fedagg_h16.hip's own loop (h16_vec.h
// clients16) with the promotions counted from row0 and the level step taken
// from n_total, and the segment either stores the planes lev_out names or,
// as the last one, finishes with the 16-bit reduce's finish (finish16: the
// sum of the levels, / n_total unless weighted, one rounding to nearest-even
// into the 16-bit bucket; a mixed plan: the fp32 value through the wide
// store).  Segments chained in slot order give the one 16-bit launch's bits.
//
// The state stays fp32: element e of level l is at state + l * plane + e.  A
// lane owns 8 adjacent columns, 32 B of every plane, read and written as two
// adjacent 16-B nt accesses (the fp32 chain's policy, reduce_impl.h POL 3).
// FA_CHAIN16_STATE_XCHG=1 builds the measured alternative instead (DESIGN
// §4.15; tools/chain16_ab.py): the wide store's pairwise lane exchange, so
// that every load and store instruction covers 1 KB contiguous per wave.
//
// Its own translation unit and its own kernels (chain16_kernel): every other
// unit's code object stays what it was.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "conv16.h"
#include "h16.h"
#include "h16_vec.h"

#ifndef FA_CHAIN16_STATE_XCHG
#define FA_CHAIN16_STATE_XCHG 0
#endif

namespace fa_chain16 {
using namespace fa_k;
using namespace fa_h16;

#if FA_CHAIN16_STATE_XCHG
// One plane's 32 B per lane through the exchange.  The wave's 64 lanes own
// fp32 vectors 2 * wv0 .. + 127 of the plane at `p` (wv0: the wave's first
// 8-column vector).  Load s reads vector 2 * wv0 + 64 s + t in lane t; lane t's
// own two vectors 2 t + h then sit in load (2 t + h) / 64, lane (2 t + h) % 64.
// Every lane takes part; a load goes out when its vector is inside the tile.
template <bool FULL>
__device__ __forceinline__ void ld_plane_x(const float* p, uint32_t wv0, uint32_t lane, int count,
                                           f4* x0, f4* x1) {
  f4 ld[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const uint32_t v = 2 * wv0 + 64 * s + lane;
    ld[s] = (FULL || (int)(4 * v) < count) ? ldg4<true>(p, v) : f4{0.f, 0.f, 0.f, 0.f};
  }
  const int s0 = (int)((2 * lane) & 63), s1 = (int)((2 * lane + 1) & 63);
  const f4 a0 = shfl4(ld[0], s0), a1 = shfl4(ld[1], s0);
  const f4 b0 = shfl4(ld[0], s1), b1 = shfl4(ld[1], s1);
  *x0 = lane < 32 ? a0 : a1;
  *x1 = lane < 32 ? b0 : b1;
}
// ... and back: store s writes vector 2 * wv0 + 64 s + t from lane t, which
// takes half t & 1 of lane 32 s + t / 2 (h16_vec.h finish16's exchange).
template <bool FULL>
__device__ __forceinline__ void st_plane_x(float* p, uint32_t wv0, uint32_t lane, int count,
                                           f4 x0, f4 x1) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int src = (int)(32 * s + (lane >> 1));
    const f4 lo = shfl4(x0, src), hi = shfl4(x1, src);
    const f4 v = (lane & 1) ? hi : lo;
    const uint32_t idx = 2 * wv0 + 64 * s + lane;
    if (FULL || (int)(4 * idx) < count) stg4<true>(p, idx, v);
  }
}
#endif

template <int EL, int U, bool FULL, bool W, bool WIDE>
__device__ __forceinline__ void tile_chain16(KArgs& a, int64_t start, int count) {
  const int n = a.n;
  const int nt = a.n_total;
  const int lp = level_power(nt);
  const int mask = (1 << lp) - 1;
  Acc<2 * U, true> A;
  uint32_t vi[U];
  bool ok[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    // block-strided: lane t takes vectors t, t + 256
    const int v = (int)threadIdx.x + u * kBlock;
    vi[u] = (uint32_t)v;
    ok[u] = FULL || kVec * v < count;
  }
#pragma unroll
  for (int j = 0; j < 2 * U; ++j)
    A.l0[j] = A.l1[j] = A.l2[j] = A.l3[j] = f4{0.f, 0.f, 0.f, 0.f};
  // the state after rows 0 .. row0 - 1: lane vector u's columns are fp32
  // vectors 2 vi[u] and 2 vi[u] + 1 of each plane
#if FA_CHAIN16_STATE_XCHG
  const uint32_t lane = threadIdx.x & 63;
  if (a.st_in) {
    const int li = a.lev_in;
    const float* s0 = a.st_in + start;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t wv0 = vi[u] - lane;
      if (li & 1) ld_plane_x<FULL>(s0, wv0, lane, count, &A.l0[2 * u], &A.l0[2 * u + 1]);
      if (li & 2) ld_plane_x<FULL>(s0 + a.plane, wv0, lane, count, &A.l1[2 * u], &A.l1[2 * u + 1]);
      if (li & 4)
        ld_plane_x<FULL>(s0 + 2 * a.plane, wv0, lane, count, &A.l2[2 * u], &A.l2[2 * u + 1]);
      if (li & 8)
        ld_plane_x<FULL>(s0 + 3 * a.plane, wv0, lane, count, &A.l3[2 * u], &A.l3[2 * u + 1]);
    }
  }
#else
  if (a.st_in) {
    const int li = a.lev_in;
    const float* s0 = a.st_in + start;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!ok[u]) continue;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint32_t v = 2 * vi[u] + h;
        if (li & 1) A.l0[2 * u + h] = ldg4<true>(s0, v);
        if (li & 2) A.l1[2 * u + h] = ldg4<true>(s0 + a.plane, v);
        if (li & 4) A.l2[2 * u + h] = ldg4<true>(s0 + 2 * a.plane, v);
        if (li & 8) A.l3[2 * u + h] = ldg4<true>(s0 + 3 * a.plane, v);
      }
    }
  }
#endif
  // the pointer source by the LOCAL count (a segment of a deep reduction may
  // hold few clients); the level step by n_total
  if (n <= kInline) clients16<EL, U, FULL, W, false>(a, A, n, start, vi, ok, lp, mask, a.row0);
  else clients16<EL, U, FULL, W, true>(a, A, n, start, vi, ok, lp, mask, a.row0);
#if FA_CHAIN16_STATE_XCHG
  if (a.st_out) {
    const int lo = a.lev_out;
    float* s0 = a.st_out + start;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t wv0 = vi[u] - lane;
      if (lo & 1) st_plane_x<FULL>(s0, wv0, lane, count, A.l0[2 * u], A.l0[2 * u + 1]);
      if (lo & 2) st_plane_x<FULL>(s0 + a.plane, wv0, lane, count, A.l1[2 * u], A.l1[2 * u + 1]);
      if (lo & 4)
        st_plane_x<FULL>(s0 + 2 * a.plane, wv0, lane, count, A.l2[2 * u], A.l2[2 * u + 1]);
      if (lo & 8)
        st_plane_x<FULL>(s0 + 3 * a.plane, wv0, lane, count, A.l3[2 * u], A.l3[2 * u + 1]);
    }
    return;
  }
#else
  if (a.st_out) {
    const int lo = a.lev_out;
    float* s0 = a.st_out + start;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!ok[u]) continue;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint32_t v = 2 * vi[u] + h;
        if (lo & 1) stg4<true>(s0, v, A.l0[2 * u + h]);
        if (lo & 2) stg4<true>(s0 + a.plane, v, A.l1[2 * u + h]);
        if (lo & 4) stg4<true>(s0 + 2 * a.plane, v, A.l2[2 * u + h]);
        if (lo & 8) stg4<true>(s0 + 3 * a.plane, v, A.l3[2 * u + h]);
      }
    }
    return;
  }
#endif
  // FA_F_SUM_ONLY reaches here on a mixed plan only (the entry refuses it on
  // a 16-bit result)
  const bool sum_only = W || (WIDE && (a.flags & FA_F_SUM_ONLY));
  finish16<EL, U, FULL, WIDE>(a, A, start, count, vi, ok, sum_only, (float)nt);
}

// One workgroup per tile; the plan holds vector tiles only.
template <int EL, int U, bool W, bool WIDE>
__global__ __launch_bounds__(kBlock) void chain16_kernel(ReduceArgs args) {
  (void)args;
  KArgs& a = *(KArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  const Tile t = a.tiles[blockIdx.x];
  if (t.kind != K_F32_VEC) return;
  if (t.count == U * kTile) tile_chain16<EL, U, true, W, WIDE>(a, t.start, t.count);
  else tile_chain16<EL, U, false, W, WIDE>(a, t.start, t.count);
}

template <int EL, int U, bool WIDE>
static hipError_t launch_w(const ReduceArgs& a, int ntiles, bool w, hipStream_t st) {
  if (w)
    hipLaunchKernelGGL((chain16_kernel<EL, U, true, WIDE>), dim3(ntiles), dim3(kBlock), 0, st, a);
  else
    hipLaunchKernelGGL((chain16_kernel<EL, U, false, WIDE>), dim3(ntiles), dim3(kBlock), 0, st, a);
  return hipGetLastError();
}
template <int EL>
static hipError_t launch_u(const ReduceArgs& a, int ntiles, int u, bool w, bool wide,
                           hipStream_t st) {
  if (wide)
    return u == 1 ? launch_w<EL, 1, true>(a, ntiles, w, st) : launch_w<EL, 2, true>(a, ntiles, w, st);
  return u == 1 ? launch_w<EL, 1, false>(a, ntiles, w, st) : launch_w<EL, 2, false>(a, ntiles, w, st);
}

hipError_t launch(const ReduceArgs& a, int ntiles, int elem, int u, bool weighted, bool wide,
                  hipStream_t st) {
  if (ntiles <= 0) return hipSuccess;
  if (elem == FA_ELEM_F16) return launch_u<FA_ELEM_F16>(a, ntiles, u, weighted, wide, st);
  if (elem == FA_ELEM_BF16) return launch_u<FA_ELEM_BF16>(a, ntiles, u, weighted, wide, st);
  return hipErrorInvalidValue;
}

}  // namespace fa_chain16
