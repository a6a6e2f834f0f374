// fedagg_h16.hip — the reduce over fp16 / bf16 buckets (model.half() /
// model.bfloat16() clients; fa_plan_create_elem).  The reference's line,
//
//     torch.stack([m.state_dict()[k].float() for m in clients], 0).mean(0)
//
// followed by load_state_dict's copy_ into the 16-bit key: every value is
// widened exactly to fp32, summed in fp32 in torch's CPU order (the orders of
// reduce_impl.h, unchanged), divided by N, and the fp32 mean rounded to
// nearest-even into the key's type.  The kernels read the clients' 16-bit
// buckets directly — half the bytes of the fp32 staging this replaces — and
// write a 16-bit result.  WIDE instances (fa_plan_create_elem_out, an fp32
// master global over 16-bit clients) store the fp32 mean unrounded into an
// fp32 bucket at the same element offsets; bcast_narrow_kernel then rounds
// that bucket into every client's 16-bit one.
//
// Vector tiles: each lane owns 8 adjacent columns per 16-B load (U loads per
// client: tiles of U * 2048 elements) and walks the clients serially with
// the next client's loads issued before the current client's adds
// (reduce_impl.h pipe2_clients' rhythm: one client in flight per wave).  All
// four cascade levels are carried at every N: levels 2-3 stay +0 below 256
// clients and x + (+0) == x for every value a +0-seeded sum can hold.
// Scalar columns (ILP-4 tails, M == 1 keys, unaligned or 4-column cascade
// bodies, int64 keys) run reduce_impl.h's cascade_seq / ilp4_seq / inner_seq
// from an LDS stage filled through a 16-bit source.
//
// Its own translation unit and its own kernel family: reduce_impl.h's fp32
// kernels are not templated on the element type (code a launch never runs
// cost other instances 0.7-2.5 %).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "common.h"
#include "conv16.h"
#include "h16.h"
#include "h16_vec.h"

namespace fa_h16 {
using namespace fa_k;

// (ldu4, st_sc1, st_sc1_f4, shfl4, the pointer sources cptr16 / cw16 and the
// client loop clients16: h16_vec.h, shared with the chain segments of
// fedagg_chain16.hip)

// --------------------------------------------------------- vector tiles ----
template <int EL, int U, bool FULL, bool W, bool WIDE>
__device__ __forceinline__ void tile_vec16(KArgs& a, int64_t start, int count) {
  const int n = a.n;
  const int lp = level_power(n);
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
  if (n <= kInline) clients16<EL, U, FULL, W, false>(a, A, n, start, vi, ok, lp, mask, 0);
  else clients16<EL, U, FULL, W, true>(a, A, n, start, vi, ok, lp, mask, 0);
  const float fn = (float)n;
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
        r[h] = W ? s : div4s(s, fn);
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
      r[h] = W ? s : div4s(s, fn);
    }
    st_sc1(out, vi[u],
           u4{narrow2<EL>(r[0].x, r[0].y), narrow2<EL>(r[0].z, r[0].w),
              narrow2<EL>(r[1].x, r[1].y), narrow2<EL>(r[1].z, r[1].w)});
  }
}

// -------------------------------------------------------- scalar columns ---
// The value each order reads from a 16-bit bucket: widened, and in a
// weighted call multiplied by the client's weight (rounded before any add).
template <int EL>
struct SrcH16 {
  KArgs& a;
  bool weighted;
  __device__ float operator()(int i, int64_t e) const {
    const float x = widen<EL>(((const uint16_t*)cptr32(a, i))[e]);
    return weighted ? __fmul_rn(x, cw(a, i)) : x;
  }
};

// reduce_impl.h scalar_column with a 16-bit result for the floating kinds
// (WIDE: the fp32 value itself into the fp32 bucket).
template <int EL, bool W, bool WIDE, class SrcF, class SrcI>
__device__ __forceinline__ void scalar_column16(KArgs& a, const SrcF& sf, const SrcI& si,
                                                int64_t e, int kind) {
  const int n = a.n;
  const float fn = (float)n;
  if (kind <= K_F32_INNER) {
    float s;
    if (kind == K_F32_CASC_S) s = cascade_seq(sf, e, 0, 1, n);
    else if (kind == K_F32_ILP4) s = ilp4_seq(sf, e, 0, 1, n);
    else s = inner_seq(sf, e, n);
    s = __fadd_rn(0.f, s);  // sum_out: out (=+0) += value
    const float r = W ? s : __fdiv_rn(s, fn);
    if constexpr (WIDE) a.out32[e] = r;
    else ((uint16_t*)a.out32)[e] = (uint16_t)narrow<EL>(r);
  } else {
    float s;
    if (kind == K_I64_CASC) s = cascade_seq(si, e, 0, 1, n);
    else if (kind == K_I64_ILP4) s = ilp4_seq(si, e, 0, 1, n);
    else s = inner_seq(si, e, n);
    s = __fadd_rn(0.f, s);
    a.out64[e] = (int64_t)__fdiv_rn(s, fn);  // copy_: fp32 -> int64 truncates
  }
}

// reduce_impl.h tile_scalar_packed over a 16-bit floating bucket: packed tile
// k's up to kPackCols columns (entries at sidx[k * kPackCols ..], -1 unused),
// their N rows staged into LDS with independent loads, each column's order
// run from LDS by one lane of wave 0.
template <int EL, bool W, bool WIDE>
__device__ __forceinline__ void tile_scalar16(KArgs& a, int k) {
  __shared__ float stage[kStageFloats];
  const int n = a.n;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t* ents = a.sidx + (int64_t)k * kPackCols;
  if (n > kStageFloats) {  // direct loads, one column per lane of wave 0
    if (wv == 0) {
      const int64_t ent = ents[lane];
      if (ent >= 0)
        scalar_column16<EL, W, WIDE>(a, SrcH16<EL>{a, W}, SrcI64{a}, ent >> 4, (int)(ent & 15));
    }
    return;
  }
  const int sub = min(kPackCols, kStageFloats / n);  // columns staged at once
  for (int c0 = 0; c0 < kPackCols; c0 += sub) {
    const int m = min(sub, kPackCols - c0);
    const int64_t ent = lane < m ? ents[c0 + lane] : -1;
    const bool mine = ent >= 0;
    const int64_t e = mine ? ent >> 4 : 0;
    const int kind = mine ? (int)(ent & 15) : K_F32_ILP4;
    const bool flt = kind <= K_F32_INNER;
    constexpr int R = 8;  // rows in flight per lane
    for (int i0 = wv; i0 < n; i0 += 4 * R) {
      float x[R];
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const int r = i0 + 4 * u;
        if (r < n && mine) x[u] = flt ? SrcH16<EL>{a, W}(r, e) : SrcI64{a}(r, e);
      }
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const int r = i0 + 4 * u;
        if (r < n && mine) stage[r * m + lane] = x[u];
      }
    }
    __syncthreads();
    if (wv == 0 && mine) {
      const SrcLdsCol src{stage, m, lane};
      scalar_column16<EL, W, WIDE>(a, src, src, e, kind);
    }
    __syncthreads();
  }
}

// ----------------------------------------------------------------- kernel --
// One workgroup per tile; the packed scalar tiles lead the table.
template <int EL, int U, bool W, bool WIDE = false>
__global__ __launch_bounds__(kBlock) void h16_round_kernel(ReduceArgs args) {
  (void)args;
  KArgs& a = *(KArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  const int ti = blockIdx.x;
  if (ti < a.nscalar) {
    tile_scalar16<EL, W, WIDE>(a, ti);
    return;
  }
  const Tile t = a.tiles[ti];
  if (t.kind != K_F32_VEC) return;
  if (t.count == U * kTile) tile_vec16<EL, U, true, W, WIDE>(a, t.start, t.count);
  else tile_vec16<EL, U, false, W, WIDE>(a, t.start, t.count);
}

template <int EL, int U, bool WIDE>
static hipError_t launch_w(const ReduceArgs& a, int ntiles, bool w, hipStream_t st) {
  if (w)
    hipLaunchKernelGGL((h16_round_kernel<EL, U, true, WIDE>), dim3(ntiles), dim3(kBlock), 0, st, a);
  else
    hipLaunchKernelGGL((h16_round_kernel<EL, U, false, WIDE>), dim3(ntiles), dim3(kBlock), 0, st,
                       a);
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

// ------------------------------------------------- narrowing broadcast ----
// The mixed round's broadcast (load_state_dict of the fp32 global into each
// 16-bit client): a.out32's fp32 bucket over [0, f32_numel) rounded with
// narrow2 and written to every client's 16-bit bucket, the int64 bucket
// copied.  fedagg.hip bcast_flat2_kernel's shape: one workgroup
// per (part, group of <= G clients), groups fastest; destination pointers
// through scalar loads only; one 16-B store per lane per client, back to
// back, sc1 nt; client 0's stores unconditional in whole parts, so the source
// loads are waited for once and no later store carries a vmcnt wait.  A part
// is kTile = 2048 elements: two 16-B loads per lane, and the same 4 KB per
// client per workgroup the flat broadcast writes.  The last part also narrows
// the f32_numel % 8 trailing elements.
__device__ __forceinline__ void st_bc16(uint16_t* base, uint32_t vidx, u4 v) {
  const __amdgpu_buffer_rsrc_t r =
      __builtin_amdgcn_make_buffer_rsrc(base, (short)0, 0x7fffffff, 0x00020000);
  __builtin_amdgcn_raw_buffer_store_b128(v, r, (int)(16 * vidx), 0, 18);
}
template <int EL, int G>
__global__ __launch_bounds__(kBlock) void bcast_narrow_kernel(ReduceArgs args, uint32_t parts,
                                                              uint32_t groups, uint32_t gsize,
                                                              int64_t f32_numel,
                                                              int64_t i64_numel) {
  (void)args;
  KArgs& a = *(KArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t p = blockIdx.x / groups, g = blockIdx.x % groups;
  const int c0 = (int)(g * gsize);
  const int cnt = min(a.n - c0, (int)gsize);
  if (p < parts) {
    const int64_t nv = f32_numel / kVec;          // whole 8-element vectors
    const int64_t vb = (int64_t)p * kBlock;       // the part's first vector
    const float* src = a.out32 + kVec * vb;
    const uint32_t t = threadIdx.x;
    if (vb + kBlock <= nv) {
      // (the source as one 16-B load per KB per lane and a swap of halves
      // between neighbouring lanes, so that every load and store instruction
      // covers whole KBs, measured the same: 27.9 against 27.5-27.7 us at
      // N = 5, within 1 % at N = 20 / 24)
      const u4 r = narrow8<EL>(ldg4<false>(src, 2 * t), ldg4<false>(src, 2 * t + 1));
#pragma unroll
      for (int i = 0; i < G; ++i) {
        if (i == 0 || i < cnt) st_bc16((uint16_t*)sptr32(a, c0 + i) + kVec * vb, t, r);
      }
    } else if (vb + t < nv) {
      const u4 r = narrow8<EL>(ldg4<false>(src, 2 * t), ldg4<false>(src, 2 * t + 1));
      for (int i = 0; i < cnt; ++i) st_bc16((uint16_t*)sptr32(a, c0 + i) + kVec * vb, t, r);
    }
    if (p == parts - 1 && (int64_t)t < f32_numel - kVec * nv) {
      const uint16_t x = (uint16_t)narrow<EL>(a.out32[kVec * nv + t]);
      for (int i = 0; i < cnt; ++i) ((uint16_t*)sptr32(a, c0 + i))[kVec * nv + t] = x;
    }
  } else {
    for (int64_t e = threadIdx.x; e < i64_numel; e += kBlock) {
      const int64_t x = a.out64[e];
      for (int i = 0; i < cnt; ++i) sptr64(a, c0 + i)[e] = x;
    }
  }
}

template <int EL, int G>
static void launch_bn(const ReduceArgs& a, uint32_t grid, uint32_t parts, uint32_t groups,
                      uint32_t gsize, int64_t f, int64_t i, hipStream_t st) {
  hipLaunchKernelGGL((bcast_narrow_kernel<EL, G>), dim3(grid), dim3(kBlock), 0, st, a, parts,
                     groups, gsize, f, i);
}
template <int EL>
static void launch_bg(const ReduceArgs& a, uint32_t grid, uint32_t parts, uint32_t groups,
                      uint32_t gsize, int64_t f, int64_t i, hipStream_t st) {
  if (gsize <= 8) launch_bn<EL, 8>(a, grid, parts, groups, gsize, f, i, st);
  else if (gsize <= 16) launch_bn<EL, 16>(a, grid, parts, groups, gsize, f, i, st);
  else launch_bn<EL, kBcastGroup>(a, grid, parts, groups, gsize, f, i, st);
}

hipError_t bcast_narrow(const ReduceArgs& a, int n, int elem, int64_t f32_numel,
                        int64_t i64_numel, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (elem != FA_ELEM_F16 && elem != FA_ELEM_BF16) return hipErrorInvalidValue;
  const uint32_t groups = (uint32_t)((n + kBcastGroup - 1) / kBcastGroup);
  const uint32_t gsize = (uint32_t)((n + groups - 1) / groups);
  const int64_t parts = f32_numel > 0 ? (f32_numel / kVec + kBlock - 1) / kBlock : 0;
  const int64_t fparts = f32_numel > 0 ? (parts > 0 ? parts : 1) : 0;
  const int64_t np = fparts + (i64_numel > 0 ? 1 : 0);
  if (np == 0) return hipSuccess;
  if (np * (int64_t)groups > (int64_t)UINT32_MAX) return hipErrorInvalidValue;
  const uint32_t grid = (uint32_t)(np * groups);
  if (elem == FA_ELEM_F16)
    launch_bg<FA_ELEM_F16>(a, grid, (uint32_t)fparts, groups, gsize, f32_numel, i64_numel, st);
  else
    launch_bg<FA_ELEM_BF16>(a, grid, (uint32_t)fparts, groups, gsize, f32_numel, i64_numel, st);
  return hipGetLastError();
}

// ------------------------------------------------- narrowing one range ----
// fa_narrow_f32: a range of an fp32 bucket rounded into ONE 16-bit
// destination (the chunk of a mixed host-resident round's result that goes
// back over PCIe in the clients' type, pipeline.py).  A kernel of its own:
// plain pointer arguments, no client table, no G-way store loop (the
// broadcast above is not re-templated for it).  One workgroup per kTile
// elements, two 16-B loads and one 16-B store per lane — the broadcast's
// whole-part shape, the same narrow8 / narrow bits; the last workgroup also
// narrows the numel % 8 trailing elements.  The result is read next by a
// D2H copy, not by a kernel: plain stores.
template <int EL>
__global__ __launch_bounds__(kBlock) void narrow_range_kernel(const float* __restrict__ src,
                                                              uint16_t* __restrict__ dst,
                                                              int64_t numel) {
  const int64_t nv = numel / kVec;                      // whole 8-element vectors
  const int64_t vb = (int64_t)blockIdx.x * kBlock;      // the workgroup's first vector
  const uint32_t t = threadIdx.x;
  if (vb + t < nv) {
    const float* s = src + kVec * vb;
    const u4 r = narrow8<EL>(ldg4<false>(s, 2 * t), ldg4<false>(s, 2 * t + 1));
    *((u4*)(dst + kVec * vb) + t) = r;
  }
  if (blockIdx.x == gridDim.x - 1 && (int64_t)t < numel - kVec * nv)
    dst[kVec * nv + t] = (uint16_t)narrow<EL>(src[kVec * nv + t]);
}

hipError_t narrow_range(const float* src, void* dst, int elem, int64_t numel, hipStream_t st) {
  if (numel <= 0) return hipSuccess;
  if (elem != FA_ELEM_F16 && elem != FA_ELEM_BF16) return hipErrorInvalidValue;
  const int64_t parts = std::max<int64_t>(1, (numel / kVec + kBlock - 1) / kBlock);
  if (parts > (int64_t)INT32_MAX) return hipErrorInvalidValue;
  if (elem == FA_ELEM_F16)
    hipLaunchKernelGGL(narrow_range_kernel<FA_ELEM_F16>, dim3((uint32_t)parts), dim3(kBlock), 0,
                       st, src, (uint16_t*)dst, numel);
  else
    hipLaunchKernelGGL(narrow_range_kernel<FA_ELEM_BF16>, dim3((uint32_t)parts), dim3(kBlock), 0,
                       st, src, (uint16_t*)dst, numel);
  return hipGetLastError();
}

}  // namespace fa_h16
