// fedagg.hip — MI355X (gfx950) kernels + C ABI for server-side parameter
// aggregation (the reference's server_aggregate, train_fedavg.py:138-149,
// train_fedprox.py:143-154, train_feddct.py:34-56, train_splitfed.py:34-56).
//
// The work is a bandwidth-bound column reduction: for every element of the
// flat per-client bucket, sum the N client values in exactly the order torch's
// CPU SumKernel uses (cascade / ILP-4 / 8-lane inner, see include/fedagg.h and
// DESIGN.md §2), then divide by N.  Each thread owns its columns and walks the
// clients serially, so the order costs nothing: there is no cross-lane or LDS
// reduction over clients (that would re-associate the sum).  The bucket is cut
// on the host into a tile table; one 256-thread workgroup streams one tile:
// per client, one coalesced 16-B load per lane per vector (1 KiB per wave
// instruction), loads for a batch of clients issued before their adds.
// The planners that cut the tables and the rules that pick a call's table
// and kernel form are plain host code (plan_host.cpp); this unit holds the
// kernels, the occupancy queries, the uploads, the C ABI and the launches.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared
// (no fast-math, no FTZ: the sum must be IEEE round-to-nearest-even, no FMA).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "plan_host.h"

#define FA_VERSION_STR "fedagg 0.1.0 gfx950"

// ---------------------------------------------------------------- errors --
namespace {
thread_local std::string g_last_error;
}  // namespace

int fa::set_err(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

#include "reduce_impl.h"
#include "h16.h"
#include "tgpu16.h"

// the reduce kernels' launchers are instantiated in the fedagg_k*.hip units
FA_K_UNITS(extern)

namespace {
using fa::set_err;
using namespace fa_k;
#define HIP_TRY(expr) FA_HIP_TRY(expr)


// ------------------------------------------------------ small kernels ----
__global__ void div_f32_kernel(const float* __restrict__ x, float d, float* __restrict__ out,
                               int64_t numel) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < numel;
       j += (int64_t)gridDim.x * blockDim.x)
    out[j] = __fdiv_rn(x[j], d);
}
__global__ void div_trunc_i64_kernel(const float* __restrict__ x, float d,
                                     int64_t* __restrict__ out, int64_t numel) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < numel;
       j += (int64_t)gridDim.x * blockDim.x)
    out[j] = (int64_t)__fdiv_rn(x[j], d);
}

// The round's broadcast (train_fedavg.py:148-149) after the reduce: one
// workgroup per (part, group of <= G consecutive clients), groups fastest
// (consecutive blocks), so a part's groups run side by side and its source
// is fetched once.  (r01-r03 forms — one workgroup per tile writing every
// client, 2048-float parts in groups of <= 10, per-client pointer loads
// behind a vmcnt(0) wait, XCD-contiguous groups, the broadcast fused into
// the reduce — measured and dropped; tools/bcastlab.hip,
// tools/writelab.hip, tools/roundlab.hip keep them for A/B.)
__device__ __forceinline__ void bcast_part(uint32_t v, uint32_t groups, uint32_t* p,
                                           uint32_t* g) {
  *p = v / groups;
  *g = v % groups;
}
constexpr int kBcastGroupMax = 24;  // clients per broadcast workgroup

// r04: the round's broadcast with every client pointer a scalar load
// (sptr32) and a group's G stores back to back.  The r02/r03 kernels fetched
// each destination through cptr32, which the compiler serves with an
// `s_waitcnt vmcnt(0)` before every client's stores — a wave's previous
// client's stores had to complete first (ISA checked; vmcnt counts stores on
// CDNA).  Measured on one box (tools/writelab.hip, 20 x 43.9 MB destinations
// in one slab, hashed data, profiles/r04_writelab.jsonl): a lab kernel of
// this shape 127.4 us at U = 1 with all 20 clients in one workgroup (one
// source fetch: 7.23 TB/s of B read + N*B written; a pure write of the same
// N*B 124 us = 7.08 TB/s), 134.3 us at U = 2 in groups of 10, against
// 156.2 us for the r03 product kernel of the U = 2, groups-of-10 shape.
// One workgroup per (part of 1024 floats, group of <= G clients); G is the
// template bound, the host's group size `gsize` <= G.  The int64 bucket is
// one more part.  Destination stores sc1 nt (a buffer store with those
// cache-policy bits: sc1 writes through and drops the line from the XCD's
// L2, so the launch ends with no dirty lines to write back; against nt
// stores r110 47.3 vs 47.9 us, cfg3 79.5 vs 79.8, the rest within 0.3 %).
__device__ __forceinline__ void st_bc(float* base, uint32_t vidx, f4 v) {
  const __amdgpu_buffer_rsrc_t r =
      __builtin_amdgcn_make_buffer_rsrc(base, (short)0, 0x7fffffff, 0x00020000);
  __builtin_amdgcn_raw_buffer_store_b128(v, r, (int)(16 * vidx), 0, 18);
}
template <int G>
__global__ __launch_bounds__(kBlock) void bcast_flat2_kernel(ReduceArgs args, uint32_t parts,
                                                             uint32_t groups, uint32_t gsize,
                                                             int64_t f32_numel,
                                                             int64_t i64_numel) {
  (void)args;
  constexpr int U = 1;
  KArgs& a = *(KArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  uint32_t p, g;
  bcast_part(blockIdx.x, groups, &p, &g);
  const int c0 = (int)(g * gsize);
  const int cnt = min(a.n - c0, (int)gsize);
  if (p < parts) {
    const int64_t nv = f32_numel / 4;
    const int64_t vb = (int64_t)p * U * kBlock;  // the part's first float4
    const float* src = a.out32 + 4 * vb;
    f4 r[U];
    if (vb + U * kBlock <= nv) {
      // a whole part (all but possibly the last): no per-lane predicate, and
      // client 0's stores unconditional (cnt >= 1), so the source loads are
      // waited for once there and no later store carries a vmcnt wait (the
      // waitcnt pass merges pending loads across a skipped branch)
#pragma unroll
      for (int u = 0; u < U; ++u) r[u] = ldg4<false>(src, threadIdx.x + u * kBlock);
#pragma unroll
      for (int i = 0; i < G; ++i) {
        if (i == 0 || i < cnt) {
          float* d = sptr32(a, c0 + i) + 4 * vb;
#pragma unroll
          for (int u = 0; u < U; ++u) st_bc(d, threadIdx.x + u * kBlock, r[u]);
        }
      }
    } else {
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        ok[u] = vb + threadIdx.x + u * kBlock < nv;
        if (ok[u]) r[u] = ldg4<false>(src, threadIdx.x + u * kBlock);
      }
      for (int i = 0; i < cnt; ++i) {
        float* d = sptr32(a, c0 + i) + 4 * vb;
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (ok[u]) stg4<true>(d, threadIdx.x + u * kBlock, r[u]);
      }
    }
    // the last part also copies the f32_numel % 4 trailing floats
    if (p == parts - 1 && (int64_t)threadIdx.x < f32_numel - 4 * nv) {
      const float x = a.out32[4 * nv + threadIdx.x];
      for (int i = 0; i < cnt; ++i) sptr32(a, c0 + i)[4 * nv + threadIdx.x] = x;
    }
  } else {
    for (int64_t e = threadIdx.x; e < i64_numel; e += kBlock) {
      const int64_t x = a.out64[e];
      for (int i = 0; i < cnt; ++i) sptr64(a, c0 + i)[e] = x;
    }
  }
}

// The same over the plan's tile table (plans whose segments do not cover
// the bucket, and torch-GPU-order rounds): one workgroup per (tile, group of
// <= G clients); a vector tile's U <= 4 float4 per lane load before the
// group's stores.
template <int G>
__global__ __launch_bounds__(kBlock) void bcast_group2_kernel(ReduceArgs args, uint32_t groups,
                                                              uint32_t gsize) {
  (void)args;
  KArgs& a = *(KArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  uint32_t ti, g;
  bcast_part(blockIdx.x, groups, &ti, &g);
  const int c0 = (int)(g * gsize);
  const int cnt = min(a.n - c0, (int)gsize);
  const Tile t = a.tiles[ti];
  const int kb = t.kind & 0xFF;
  if (kb == K_F32_VEC || kb == K_F32_TGPU_V || kb == K_F32_TGPU_W) {
    const uint32_t nv = (uint32_t)t.count / 4;
    f4 r[4];
    if (nv == 2 * kBlock) {
      // a full 2048-float tile (the default width): unpredicated, client 0's
      // stores unconditional (see bcast_flat2_kernel)
#pragma unroll
      for (int u = 0; u < 2; ++u) r[u] = ldg4<false>(a.out32 + t.start, threadIdx.x + u * kBlock);
#pragma unroll
      for (int i = 0; i < G; ++i) {
        if (i == 0 || i < cnt) {
          float* d = sptr32(a, c0 + i) + t.start;
#pragma unroll
          for (int u = 0; u < 2; ++u) st_bc(d, threadIdx.x + u * kBlock, r[u]);
        }
      }
      return;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t vi = threadIdx.x + u * kBlock;
      if (vi < nv) r[u] = ldg4<false>(a.out32 + t.start, vi);
    }
    for (int i = 0; i < cnt; ++i) {
      float* d = sptr32(a, c0 + i) + t.start;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t vi = threadIdx.x + u * kBlock;
        if (vi < nv) stg4<true>(d, vi, r[u]);
      }
    }
  } else if ((int)threadIdx.x < t.count) {
    int64_t e = t.start + threadIdx.x;
    bool is64 = kind_is64(t.kind);
    if (kb == K_SCALAR_PACKED) {  // a packed column: its element and kind
      const int64_t ent = a.sidx[e];
      e = ent >> 4;
      is64 = kind_is64((int)(ent & 15));
    }
    if (!is64) {
      const float x = a.out32[e];
      for (int i = 0; i < cnt; ++i) sptr32(a, c0 + i)[e] = x;
    } else {
      const int64_t x = a.out64[e];
      for (int i = 0; i < cnt; ++i) sptr64(a, c0 + i)[e] = x;
    }
  }
}

// ---------------------------------------------- torch-ROCm's GPU order ----
// The reduction torch-ROCm itself performs for stack(list, 0).mean(0) on
// device tensors (ATen/native/hip/Reduce.cuh as built into this torch:
// setReduceConfig, thread_reduce_impl, block_y_reduce / block_x_reduce;
// MeanOps: project = acc * factor) — the order of the reference's original
// GPU runs (train_fedavg.py:244-250 place the models on the GPU before
// server_aggregate).  Opt-in (fa_plan_create_order); the default order is
// torch's CPU one.
//   outer (M >= 2): rows split S ways (S = 1 or the block height bh when
//     N >= min(16*bh, 256)); part y takes rows y, y+S, ... round-robin into
//     4 accumulators from +0, combined ((a0+a1)+a2)+a3; the S parts meet in
//     block_y_reduce's halving tree; times the factor.  One element/thread.
//   inner (M == 1): lane l < bw = last_pow2(N) takes rows l, l+bw (the same
//     4-accumulator thread order), then the intra-wave tree with increasing
//     shuffle offsets (ROCm's), lane 0's value times the factor.  One
//     element per wave.
template <class Src, int S>
__device__ __forceinline__ float tgpu_outer(const Src& src, int64_t e, int n) {
  float v[S];
#pragma unroll
  for (int y = 0; y < S; ++y) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int r = y;
    for (; r + 3 * S < n; r += 4 * S) {
      a0 = __fadd_rn(a0, src(r, e));
      a1 = __fadd_rn(a1, src(r + S, e));
      a2 = __fadd_rn(a2, src(r + 2 * S, e));
      a3 = __fadd_rn(a3, src(r + 3 * S, e));
    }
    if (r < n) a0 = __fadd_rn(a0, src(r, e));
    if (r + S < n) a1 = __fadd_rn(a1, src(r + S, e));
    if (r + 2 * S < n) a2 = __fadd_rn(a2, src(r + 2 * S, e));
    v[y] = __fadd_rn(__fadd_rn(__fadd_rn(a0, a1), a2), a3);
  }
#pragma unroll
  for (int off = S / 2; off > 0; off /= 2)
#pragma unroll
    for (int y = 0; y < off; ++y) v[y] = __fadd_rn(v[y], v[y + off]);
  return v[0];
}

// The same order for 4 consecutive elements of one tensor per lane (the
// order depends only on (N, M), so the 4 lanes of a float4 are 4 independent
// copies of it): 16-B non-temporal loads, up to eight rows' loads (two
// round-robin steps) in flight per lane.  Vector adds are per-component IEEE
// adds (no multiply feeds them, so contraction cannot apply).
template <int S>
__device__ __forceinline__ f4 tgpu_outer4(KArgs& a, int64_t start, uint32_t v, int n) {
  f4 val[S];
#pragma unroll
  for (int y = 0; y < S; ++y) {
    // part y's p-th row is y + p*S; row p goes into accumulator p % 4.  Rows
    // are loaded B at a time, then added in row order, so every accumulator
    // still sees its rows in increasing order.
    const f4 z = {0.f, 0.f, 0.f, 0.f};
    f4 acc[4] = {z, z, z, z};
    const int np = (n - y + S - 1) / S;
    constexpr int B = S >= 8 ? 4 : 8;  // rows in flight (register budget of val[S])
    int p = 0;
    for (; p + B <= np; p += B) {
      f4 x[B];
#pragma unroll
      for (int i = 0; i < B; ++i) x[i] = ldg4<true>(cptr32(a, y + (p + i) * S) + start, v);
#pragma unroll
      for (int i = 0; i < B; ++i) acc[i & 3] += x[i];
    }
    if (p < np) {  // p % 4 == 0 here: row p + i goes into accumulator i & 3
      f4 x[B];
#pragma unroll
      for (int i = 0; i < B; ++i)
        if (p + i < np) x[i] = ldg4<true>(cptr32(a, y + (p + i) * S) + start, v);
#pragma unroll
      for (int i = 0; i < B; ++i)
        if (p + i < np) acc[i & 3] += x[i];
    }
    val[y] = ((acc[0] + acc[1]) + acc[2]) + acc[3];
  }
#pragma unroll
  for (int off = S / 2; off > 0; off /= 2)
#pragma unroll
    for (int y = 0; y < off; ++y) val[y] = val[y] + val[y + off];
  return val[0];
}

// S = 1 (no row split: every BASELINE config's tensors) over 2048-element
// tiles, the default kernel's load shape: U = 2 float4 per lane per row, rows
// in batches of B (a multiple of 4, so row b of a batch feeds accumulator
// b & 3 statically), loads through the same pointer accessor as the default
// reduce.  Row p goes into accumulator p % 4 in increasing row order, then
// ((a0 + a1) + a2) + a3 — torch's thread order, per component.
template <int U, int B, bool FULL, int PIPE = 0>
__device__ __forceinline__ void tgpu_wide(KArgs& a, int64_t start, int count, float fac,
                                          bool sum_only) {
  static_assert(B % 4 == 0, "batch must keep the accumulator index static");
  const f4 z = {0.f, 0.f, 0.f, 0.f};
  f4 acc[4][U];
  uint32_t vi[U];
  bool ok[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    vi[u] = threadIdx.x + u * kBlock;
    ok[u] = FULL || (int)(4 * vi[u]) < count;
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k][u] = z;
  }
  const int n = a.n;
  int b0 = 0;
  if constexpr (PIPE != 0 && FULL) {
    // the client loop (as reduce_impl.h pipe2_clients): row b + 1's loads
    // before row b's adds; four rows per pass keep row b's accumulator
    // index (b & 3) static.  The rows' order per accumulator is unchanged.
    // Pointers through scalar loads only (sptr32): cptr32's table arm is a
    // vector load, and the compiler then waited for the current row's data
    // before issuing the next row's loads (ISA read; same process -0.3 ..
    // -0.9 % on cfg2 / cfg3 / cfg5, profiles/r05_ab_lib_tgpu_sptr.jsonl).
    // Same process, r05: cfg2 order 139.9 -> 136.7 us, cfg5 169.9 -> 166.6,
    // N = 17 / 28 -2.8 / -2.5 %, cfg3 and N = 2..16 -1.3 .. +0.1 %, unlike
    // the default kernel's rule: both batch sizes take it
    f4 cur[U], nxt[U];
    {
      const float* p = sptr32(a, 0) + start;
#pragma unroll
      for (int u = 0; u < U; ++u) cur[u] = ldg4<true>(p, vi[u]);
    }
    for (; b0 < n; b0 += 4) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int b = b0 + k;
        if (b < n) {
          if (b + 1 < n) {
            const float* p = sptr32(a, b + 1) + start;
#pragma unroll
            for (int u = 0; u < U; ++u) nxt[u] = ldg4<true>(p, vi[u]);
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            acc[k][u] += cur[u];
            cur[u] = nxt[u];
          }
        }
      }
    }
  }
  for (; b0 + B <= n; b0 += B) {
    f4 x[B][U];
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const float* p = cptr32(a, b0 + b) + start;
#pragma unroll
      for (int u = 0; u < U; ++u)
        x[b][u] = (FULL || ok[u]) ? ldg4<true>(p, vi[u]) : z;
    }
#pragma unroll
    for (int b = 0; b < B; ++b)
#pragma unroll
      for (int u = 0; u < U; ++u) acc[b & 3][u] += x[b][u];
  }
  if (b0 < n) {  // b0 % 4 == 0 here
    const int nb = n - b0;
    f4 x[B][U];
#pragma unroll
    for (int b = 0; b < B; ++b) {
      if (b < nb) {
        const float* p = cptr32(a, b0 + b) + start;
  #pragma unroll
        for (int u = 0; u < U; ++u)
          x[b][u] = (FULL || ok[u]) ? ldg4<true>(p, vi[u]) : z;
      }
    }
#pragma unroll
    for (int b = 0; b < B; ++b)
      if (b < nb)
#pragma unroll
        for (int u = 0; u < U; ++u) acc[b & 3][u] += x[b][u];
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (!FULL && !ok[u]) continue;
    f4 r = ((acc[0][u] + acc[1][u]) + acc[2][u]) + acc[3][u];
    if (!sum_only)
      r = f4{__fmul_rn(r.x, fac), __fmul_rn(r.y, fac), __fmul_rn(r.z, fac), __fmul_rn(r.w, fac)};
    st_out<5>(a.out32, start, vi[u], r);  // sc1: see reduce_impl.h st_out
  }
}

// S = 1 or 2 (torch's row split for N >= 32 over the large tensors) over
// 2048-element tiles with the client loop: rows in slot order, row r into
// part r % S and that part's accumulator (r / S) % 4 — part y's p-th row
// (y + S p) into accumulator p % 4, as tgpu_outer4<S> — then each part's
// ((a0 + a1) + a2) + a3 and, for S = 2, part 0 + part 1.  4 S rows per pass
// keep the accumulator index static.  The S = 2 launch runs its S = 1 tiles
// through it too (tgpu_kernel<1>).
// FA_TGPU_LOOP_DEPTH: rows in flight ahead of the add (1: row b + 1's loads
// before row b's adds).  2 and 3 (same 130 VGPRs, three workgroups per CU)
// measured within +-0.4 % of 1 at N = 32 / 48 / 64 (r06,
// profiles/r06_ab_lib_tgpu_runs.jsonl): the launch is not short of loads in
// flight.
#ifndef FA_TGPU_LOOP_DEPTH
#define FA_TGPU_LOOP_DEPTH 1
#endif
template <int U, int S, bool FULL>
__device__ __forceinline__ void tgpu_wide_loop(KArgs& a, int64_t start, int count, float fac,
                                               bool sum_only) {
  static_assert(S == 1 || S == 2, "row split of the wide loop");
  constexpr int R = 4 * S;
  constexpr int D = FA_TGPU_LOOP_DEPTH;
  const f4 z = {0.f, 0.f, 0.f, 0.f};
  f4 acc[R][U];
  uint32_t vi[U];
  bool ok[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    vi[u] = threadIdx.x + u * kBlock;
    ok[u] = FULL || (int)(4 * vi[u]) < count;
#pragma unroll
    for (int k = 0; k < R; ++k) acc[k][u] = z;
  }
  const int n = a.n;
  f4 row[D + 1][U];   // row[0]: the row being added; row[d]: d rows ahead
#pragma unroll
  for (int d = 0; d < D; ++d) {
    if (d < n) {
      const float* p = sptr32(a, d) + start;
#pragma unroll
      for (int u = 0; u < U; ++u) row[d][u] = (FULL || ok[u]) ? ldg4<true>(p, vi[u]) : z;
    }
  }
  for (int b0 = 0; b0 < n; b0 += R) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int b = b0 + k;
      if (b < n) {
        if (b + D < n) {
          const float* p = sptr32(a, b + D) + start;
#pragma unroll
          for (int u = 0; u < U; ++u) row[D][u] = (FULL || ok[u]) ? ldg4<true>(p, vi[u]) : z;
        }
        const int ai = (k % S) * 4 + ((k / S) & 3);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          acc[ai][u] += row[0][u];
#pragma unroll
          for (int d = 0; d < D; ++d) row[d][u] = row[d + 1][u];
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (!FULL && !ok[u]) continue;
    f4 r = ((acc[0][u] + acc[1][u]) + acc[2][u]) + acc[3][u];
    if constexpr (S == 2) r = r + (((acc[4][u] + acc[5][u]) + acc[6][u]) + acc[7][u]);
    if (!sum_only)
      r = f4{__fmul_rn(r.x, fac), __fmul_rn(r.y, fac), __fmul_rn(r.z, fac), __fmul_rn(r.w, fac)};
    st_out<5>(a.out32, start, vi[u], r);
  }
}

// lane value of the inner order; the wave then runs the shuffle tree
template <class Src>
__device__ __forceinline__ float tgpu_inner(const Src& src, int64_t e, int n, int bw, int lane) {
  float a0 = 0.f, a1 = 0.f;
  if (lane < n) a0 = __fadd_rn(a0, src(lane, e));
  if (lane + bw < n) a1 = __fadd_rn(a1, src(lane + bw, e));
  float v = __fadd_rn(__fadd_rn(__fadd_rn(a0, a1), 0.f), 0.f);
  for (int off = 1; off < bw; off <<= 1) v = __fadd_rn(v, __shfl_down(v, off, 64));
  return v;
}

// M == 1 with N >= 128: torch vectorises along the input (setReduceConfig's
// "vectorize along input": dim0 = N / 4 >= 32), so the block is bw =
// last_pow2(N / 4) (at most 512) threads; thread x sums the 4-element
// vectors x, x+bw, ... into 4 accumulators, one per vector component, then
// the <= 3 trailing rows N - N%4 + x into accumulator 0, and combines
// ((v0 + v1) + v2) + v3 (input_vectorized_thread_reduce_impl).  The threads
// meet in block_x_reduce: the shared-memory halving tree for offsets bw/2
// down to 64, then the intra-wave tree with increasing offsets.  One wave per
// element here: lane l plays threads l + 64 j (j < bw / 64), and the halving
// over j is the shared-memory tree.
template <class Src>
__device__ __forceinline__ float tgpu_inner_vec(const Src& src, int64_t e, int n, int bw,
                                                int lane) {
  const int J = bw >= 64 ? bw / 64 : 1;
  const int tail = n - n % 4;
  float t[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    t[j] = 0.f;
    const int x = lane + 64 * j;
    if (j >= J || x >= bw) continue;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
    for (int q = x; 4 * q + 3 < n; q += bw) {
      v0 = __fadd_rn(v0, src(4 * q, e));
      v1 = __fadd_rn(v1, src(4 * q + 1, e));
      v2 = __fadd_rn(v2, src(4 * q + 2, e));
      v3 = __fadd_rn(v3, src(4 * q + 3, e));
    }
    if (tail + x < n) v0 = __fadd_rn(v0, src(tail + x, e));
    t[j] = __fadd_rn(__fadd_rn(__fadd_rn(v0, v1), v2), v3);
  }
  if (J >= 8) {
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = __fadd_rn(t[j], t[j + 4]);
  }
  if (J >= 4) {
#pragma unroll
    for (int j = 0; j < 2; ++j) t[j] = __fadd_rn(t[j], t[j + 2]);
  }
  if (J >= 2) t[0] = __fadd_rn(t[0], t[1]);
  float v = t[0];
  const int dx = bw >= 64 ? 64 : bw;
  for (int off = 1; off < dx; off <<= 1) v = __fadd_rn(v, __shfl_down(v, off, 64));
  return v;
}

// A V tile (4 elements per lane) and a scalar tile (one element per lane)
// of row split S.
template <int S>
__device__ __forceinline__ void tgpu_v_tile(KArgs& a, const Tile& t, float fac, bool sum_only) {
  const uint32_t v = threadIdx.x;
  if ((int)(v * 4) >= t.count) return;
  f4 r = tgpu_outer4<S>(a, t.start, v, a.n);
  if (!sum_only)
    r = f4{__fmul_rn(r.x, fac), __fmul_rn(r.y, fac), __fmul_rn(r.z, fac), __fmul_rn(r.w, fac)};
  st_out<5>(a.out32, t.start, v, r);
}
template <int S>
__device__ __forceinline__ void tgpu_scalar_tile(KArgs& a, const Tile& t, float fac,
                                                 bool sum_only) {
  const int j = threadIdx.x;
  if (j >= t.count) return;
  const int64_t e = t.start + j;
  if ((t.kind & 0xFF) == K_F32_TGPU) {
    const float s = tgpu_outer<SrcF32, S>(SrcF32{a, false}, e, a.n);
    a.out32[e] = sum_only ? s : __fmul_rn(s, fac);
  } else {
    a.out64[e] = (int64_t)__fmul_rn(tgpu_outer<SrcI64, S>(SrcI64{a}, e, a.n), fac);
  }
}

// One instantiation per row split S = 1 << LS (the plan groups its tiles by
// S and launches each group): a single S per kernel keeps the register
// budget of the parts' values to that S (a runtime switch over S = 1..16 in
// one kernel needed 300 VGPRs and spilled).  Inner tiles (M == 1) ride in
// the LS = 0 group; their own field is the lane count exponent.  r05: when
// the S = 2 group is the largest (N >= 32 over the large tensors) the S = 1
// and S = 4 tiles and the inner tiles ride in its launch (their own S from
// the tile's field; fa_plan_create_order), so the small groups cost no
// launch of their own.
template <int LS, int WB = 16, int PIPE = 0>
__global__ __launch_bounds__(kBlock) void tgpu_kernel(ReduceArgs args) {
  (void)args;
  constexpr int S = 1 << LS;
  KArgs& a = *(KArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  const Tile t = a.tiles[blockIdx.x];
  const float fac = a.tfac[blockIdx.x];
  const int base = t.kind & 0xFF, ls = (t.kind >> 8) & 0xFF;
  const bool sum_only = a.flags & FA_F_SUM_ONLY;
  const int n = a.n;
  const bool inner = base == K_F32_TGPU_IN || base == K_I64_TGPU_IN;
  if constexpr (LS == 0) {
    if (base == K_F32_TGPU_W) {
      if (t.count == 8 * kBlock) tgpu_wide<2, WB, true, PIPE>(a, t.start, t.count, fac, sum_only);
      else tgpu_wide<2, WB, false>(a, t.start, t.count, fac, sum_only);
      return;
    }
  }
  if constexpr (LS == 1) {
    if (base == K_F32_TGPU_W) {
      if (ls == 0) {
        if (t.count == 8 * kBlock) tgpu_wide_loop<2, 1, true>(a, t.start, t.count, fac, sum_only);
        else tgpu_wide_loop<2, 1, false>(a, t.start, t.count, fac, sum_only);
      } else {
        if (t.count == 8 * kBlock) tgpu_wide_loop<2, 2, true>(a, t.start, t.count, fac, sum_only);
        else tgpu_wide_loop<2, 2, false>(a, t.start, t.count, fac, sum_only);
      }
      return;
    }
    if (!inner && ls != 1) {  // a rider: S = 1 or 4
      if (base == K_F32_TGPU_V) tgpu_v_tile<4>(a, t, fac, sum_only);
      else if (ls == 0) tgpu_scalar_tile<1>(a, t, fac, sum_only);
      else tgpu_scalar_tile<4>(a, t, fac, sum_only);
      return;
    }
  }
  if (base == K_F32_TGPU_V) {
    tgpu_v_tile<S>(a, t, fac, sum_only);
    return;
  }
  if (base == K_F32_TGPU || base == K_I64_TGPU) {
    tgpu_scalar_tile<S>(a, t, fac, sum_only);
    return;
  }
  // inner: one element per wave
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (w >= t.count) return;
  const int64_t e = t.start + w;
  const int bw = 1 << ls;
  const bool vec = (t.kind >> 16) & 1;   // N >= 128: input-vectorised form
  if (base == K_F32_TGPU_IN) {
    const float s = vec ? tgpu_inner_vec(SrcF32{a, false}, e, n, bw, lane)
                        : tgpu_inner(SrcF32{a, false}, e, n, bw, lane);
    if (lane == 0) a.out32[e] = sum_only ? s : __fmul_rn(s, fac);
  } else {
    const float s = vec ? tgpu_inner_vec(SrcI64{a}, e, n, bw, lane)
                        : tgpu_inner(SrcI64{a}, e, n, bw, lane);
    if (lane == 0) a.out64[e] = (int64_t)__fmul_rn(s, fac);
  }
}

// fa_broadcast_f32: up to kBcastInline destinations per launch, pointers in
// the kernel arguments (more destinations: consecutive launches, each
// re-reading the source)
constexpr int kBcastInline = 256;
struct BcastArgs {
  const float* src;
  int n;
  float* dst[kBcastInline];
};
// One workgroup per (2048-float part, group of <= kBcastGroupMax
// destinations), groups fastest; the last part also copies the numel % 4
// tail.
__global__ __launch_bounds__(kBlock) void bcast_kernel(BcastArgs a, int64_t numel,
                                                       uint32_t parts, uint32_t groups,
                                                       uint32_t gsize) {
  const int64_t nv = numel / 4;
  const uint32_t total = parts * groups;
  for (uint32_t v = blockIdx.x; v < total; v += gridDim.x) {
    uint32_t p, g;
    bcast_part(v, groups, &p, &g);
    const int c0 = (int)(g * gsize);
    const int c1 = min(a.n, c0 + (int)gsize);
    const int64_t v0 = (int64_t)p * 2 * kBlock + threadIdx.x, v1 = v0 + kBlock;
    f4 r0 = {0.f, 0.f, 0.f, 0.f}, r1 = r0;
    if (v0 < nv) r0 = ld4<false>(a.src + 4 * v0);
    if (v1 < nv) r1 = ld4<false>(a.src + 4 * v1);
    for (int c = c0; c < c1; ++c) {
      if (v0 < nv) st4<true>(a.dst[c] + 4 * v0, r0);
      if (v1 < nv) st4<true>(a.dst[c] + 4 * v1, r1);
    }
    if (p == parts - 1 && threadIdx.x < numel - 4 * nv)
      for (int c = c0; c < c1; ++c) a.dst[c][4 * nv + threadIdx.x] = a.src[4 * nv + threadIdx.x];
  }
}

// Streaming copy (the roofline's calibration): one 16-B non-temporal load and
// store per lane, one 256-lane tile per workgroup, no loop — the fastest of
// the copy forms measured (tools/archive/copylab.hip, profiles/r02_copylab.jsonl:
// 6.62-6.66 TB/s on 1 GiB, against 5.0 TB/s for a grid-stride loop with one
// float4 per lane and 4.4-5.2 TB/s with four in flight per lane).
__global__ __launch_bounds__(kBlock) void copy_kernel(const float* __restrict__ src,
                                                      float* __restrict__ dst, int64_t numel) {
  const int64_t nv = numel / 4;
  const int64_t v = blockIdx.x * (int64_t)kBlock + threadIdx.x;
  if (v < nv) st4<true>(dst + 4 * v, ld4<true>(src + 4 * v));
  if (blockIdx.x == 0 && threadIdx.x < numel - 4 * nv)
    dst[4 * nv + threadIdx.x] = src[4 * nv + threadIdx.x];
}

// Read-only streaming probe: per workgroup sum of its float4s (calibrates the
// read-bandwidth ceiling the reduce kernel, 95 % reads, is measured against).
__global__ __launch_bounds__(kBlock) void read_probe_kernel(const float* __restrict__ src,
                                                            int64_t nv, float* __restrict__ out) {
  f4 acc = f4{0.f, 0.f, 0.f, 0.f};
  int64_t v = blockIdx.x * (int64_t)kBlock + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (; v + 3 * stride < nv; v += 4 * stride) {
    const f4 a = ld4<true>(src + 4 * v), b = ld4<true>(src + 4 * (v + stride));
    const f4 c = ld4<true>(src + 4 * (v + 2 * stride)), d = ld4<true>(src + 4 * (v + 3 * stride));
    acc += (a + b) + (c + d);
  }
  for (; v < nv; v += stride) acc += ld4<true>(src + 4 * v);
  float s = acc.x + acc.y + acc.z + acc.w;
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(out + blockIdx.x, s);
}

// Write-only probe in the round broadcast's own shape (fa_write_probe_f32,
// r04): one workgroup per (1024-float part, group of <= kBcastGroupMax
// destinations, as bcast_flat2_kernel), one 16-B store per lane per
// destination with the broadcast's sc1 nt policy, the
// values non-zero and non-repeating (an integer hash of the element index
// and `seed`, computed in registers: nothing is read).  Zero-filled or
// constant stores are no write ceiling on this chip.
__device__ __forceinline__ float probe_val(uint32_t i) {
  i ^= i >> 16;
  i *= 0x7feb352du;
  i ^= i >> 15;
  i *= 0x846ca68bu;
  i ^= i >> 16;
  return __fmul_rn((float)(int32_t)((i >> 8) | 1u) - 8388608.0f, 1.0f / 8388608.0f);
}
__global__ __launch_bounds__(kBlock) void write_probe_kernel(BcastArgs a, int64_t numel,
                                                             uint32_t parts, uint32_t groups,
                                                             uint32_t gsize, uint32_t seed) {
  uint32_t p, g;
  bcast_part(blockIdx.x, groups, &p, &g);
  const int c0 = (int)(g * gsize);
  const int c1 = min(a.n, c0 + (int)gsize);
  const int64_t nv = numel / 4;
  const int64_t v = (int64_t)p * kBlock + threadIdx.x;
  if (v >= nv) return;
  const uint32_t b = (uint32_t)(4 * v) ^ seed;
  const f4 x = {probe_val(b), probe_val(b + 1), probe_val(b + 2), probe_val(b + 3)};
  // based at the part's start, as bcast_flat2_kernel: the buffer offset is
  // 32-bit, so a bucket-based offset would wrap past 2^28 float4s
  for (int c = c0; c < c1; ++c) st_bc(a.dst[c] + 4 * (int64_t)p * kBlock, threadIdx.x, x);
}

// Read-only probe in the reduce's own shape (grid = 0 in fa_read_probe_f32):
// one tile of 2 x 1024 floats per workgroup, 2 independent 16-B
// non-temporal loads per lane, no loop, and no store unless the tile's sum
// hits a sentinel value (so nothing but the reads reaches HBM).  The lab's
// fastest read-only form (tools/archive/bwlab.hip one_stream_read_only_U2: 7.0-7.1
// TB/s, profiles/r01_bwlab.jsonl) — the read ceiling of a box, which the
// reduce (95 % reads) is compared with; the grid-stride form above runs
// ~10 % slower.
__global__ __launch_bounds__(kBlock) void read_tile_kernel(const float* __restrict__ src,
                                                           int64_t nv, float* __restrict__ out) {
  const int64_t v0 = blockIdx.x * (int64_t)(2 * kBlock) + threadIdx.x, v1 = v0 + kBlock;
  f4 a = f4{0.f, 0.f, 0.f, 0.f}, b = a;
  if (v0 < nv) a = ld4<true>(src + 4 * v0);
  if (v1 < nv) b = ld4<true>(src + 4 * v1);
  const f4 s = a + b;
  if (s.x == 1234.5f && s.y == -1.0f && s.z == 7.0f) out[threadIdx.x] = s.w;
}

// ------------------------------------------- synthetic state (synth.py) --
__device__ __forceinline__ uint64_t hash64(uint64_t seed, uint64_t idx) {
  uint64_t z = seed * 0x9E3779B97F4A7C15ull + idx * 0xD1B54A32D192ED03ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ float sym_unit(uint64_t h) {
  const int64_t v = (int64_t)(h >> 40) - (1 << 23);
  return __fmul_rn((float)v, 1.0f / 8388608.0f);
}
constexpr uint64_t kBaseSeed = 7, kClientSeed0 = 1000;
constexpr int kKeyShift = 36;

__global__ void synth_f32_kernel(float* dst, int64_t numel, int key, int client,
                                 float mu, float sigma, float dsig, int mode) {
  const uint64_t kb = (uint64_t)key << kKeyShift;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < numel;
       j += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t idx = kb | (uint64_t)j;
    const uint64_t hc = hash64(kClientSeed0 + client, idx);
    float x;
    if (mode == 1) {
      const int ex = (int)((hc >> 8) % 41ull) - 20;
      x = __fmul_rn(sym_unit(hc), ldexpf(1.0f, ex));
    } else {
      const float base = __fadd_rn(mu, __fmul_rn(sigma, sym_unit(hash64(kBaseSeed, idx))));
      x = __fadd_rn(base, __fmul_rn(dsig, sym_unit(hc)));
    }
    dst[j] = x;
  }
}
__global__ void synth_i64_kernel(int64_t* dst, int64_t numel, int key, int client, int mode) {
  const uint64_t kb = (uint64_t)key << kKeyShift;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < numel;
       j += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t hc = hash64(kClientSeed0 + client, kb | (uint64_t)j);
    dst[j] = mode == 1 ? (int64_t)(hc % (1ull << 26)) - (1ll << 25)
                       : (int64_t)(19 * 5) + (int64_t)(hc % 7ull);
  }
}

// ------------------------------------------------------------ host plan --
int grid_for(int64_t work, int per_block) {
  int64_t g = (work + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > 256 * 16) g = 256 * 16;
  return (int)g;
}

}  // namespace

// The kernel family a plan's calls launch, recorded once at creation: the
// default fp32 reduce, the 16-bit reduce (fedagg_h16.hip; a mixed plan's
// wide-store instances too), and the torch-GPU order over fp32 (tgpu_kernel)
// and over 16-bit buckets (fedagg_tgpu16.hip).
enum class FaFamily : int { kDefault = 0, kH16 = 1, kTgpu = 2, kTgpu16 = 3 };

// The plan's host summary — device, flags, vec_u, and the device tables' own
// counts nt / ns / nt_alt / ns_alt / bal[] (their scalar tiles are packed,
// r03, K_SCALAR_PACKED; info.* keep the host view of the layout's tiles) —
// is the launch rules' input (fa_host::PlanShape); the device pointers are
// held here.
struct fa_plan : fa_host::PlanShape {
  Tile* d_tiles = nullptr;
  fa_plan_info info{};
  // auto plans (tile_elems == 0) also carry a 1024-float table, used for
  // unweighted reductions over 129..255 clients (fa_host::select_launch)
  Tile* d_tiles_alt = nullptr;
  int64_t* d_sidx = nullptr;  // packed scalar columns: (element << 4) | kind, -1 unused
  int64_t sidx_alt_off = 0;   // the alt table's region of d_sidx
  // balanced tables (r03), bal[i]'s tiles: the vector tiles re-cut so that
  // packed + vector tiles fill whole rounds of `slots` resident workgroups
  // (balance_vec); their packed tiles are the main table's (same scalar
  // index region)
  std::vector<Tile*> d_bal;
  bool has32 = false;  // the tile table touches the fp32 bucket
  bool has64 = false;  // ... the int64 bucket
  // element type of the floating bucket (fa_plan_create_elem).  A 16-bit
  // plan holds the plain table only (no alt, no balanced tables), info and
  // tiles in 16-bit elements, vec_u = 16-B loads per lane per client
  int elem = FA_ELEM_F32;
  // element type of the result bucket (fa_plan_create_elem_out).  == elem but
  // on a mixed plan: 16-bit clients, FA_ELEM_F32 result (the fp32 master
  // global), the wide-store reduce and the narrowing broadcast
  int out_elem = FA_ELEM_F32;
  FaFamily family = FaFamily::kDefault;
  bool tgpu() const { return family == FaFamily::kTgpu || family == FaFamily::kTgpu16; }
  int order_n = 0;        // the torch-GPU order: the client count it was cut for
  int tgpu_batch = 16;    // ... rows per load batch of its S = 1 tiles (8 for N < 16)
  size_t tgpu_s2_lds = 0;  // ... the S = 2 launch's LDS reservation (tgpu_s2_lds)
  float* d_fac = nullptr; // ... and its per-tile mean factors
  int tg_lo[6] = {0, 0, 0, 0, 0, 0};  // ... tiles grouped by row split S = 1..16
  // cut from a segment list with FA_PLAN_GAPS_ARE_PADDING: every byte of
  // the buckets is a tensor's or padding, so the broadcast may copy them flat
  bool flat_bcast = false;
};

namespace {
void set_kinds(fa_plan* p, const std::vector<Tile>& t) {
  for (const Tile& x : t) (kind_is64(x.kind) ? p->has64 : p->has32) = true;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// Per-device memo of what the planners ask of a device, computed once per
// process under one lock: `key` names the question (a user's tag plus its
// own index), `value()` answers it.
enum : int { kMemoReduce = 0, kMemoTgpu = 1 << 12, kMemoTgpu16 = 2 << 12, kMemoS2Lds = 3 << 12 };
template <class F>
int64_t dev_memo(int dev, int key, F value) {
  static std::mutex mu;
  static std::map<std::pair<int, int>, int64_t> cache;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find({dev, key});
  if (it != cache.end()) return it->second;
  return cache[{dev, key}] = value();
}
// Resident workgroups of a kernel on `dev`: `occ()`, its workgroups per CU,
// times the CU count (0: unknown).
template <class F>
int memo_slots(int dev, int key, F occ) {
  return (int)dev_memo(dev, key, [&]() -> int64_t {
    const int per_cu = occ();
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      cus = 0;
    return per_cu > 0 && cus > 0 ? per_cu * cus : 0;
  });
}

// ... of the reduce kernel (U, B, deep, weighted) (0 -> the plain table).
int kernel_slots(int dev, int u, int b, bool deep, bool w) {
  return memo_slots(dev, kMemoReduce + ((u * 32 + b) * 2 + deep) * 2 + w, [&] {
    switch (u * 100 + b) {
      case 108: return occupancy_u<1, 8>(deep, w);
      case 116: return occupancy_u<1, 16>(deep, w);
      case 208: return occupancy_u<2, 8>(deep, w);
      case 216: return occupancy_u<2, 16>(deep, w);
      case 408: return occupancy_u<4, 8>(deep, w);
      default: return 0;
    }
  });
}

// ... of tgpu_kernel<0> (the fp32 torch-GPU order's S = 1 group's launch).
int tgpu_slots(int dev, int batch) {
  return memo_slots(dev, kMemoTgpu + (batch == 8), [&] {
    int occ = 0;
    const hipError_t e =
        batch == 8 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, tgpu_kernel<0, 8, 1>, kBlock, 0)
                   : hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, tgpu_kernel<0, 16, 1>, kBlock, 0);
    return e == hipSuccess ? occ : 0;
  });
}

// ... of the 16-bit S = 1 group's kernel (fedagg_tgpu16.hip), by element
// type and store width.
int tgpu16_slots(int dev, int elem, bool wide) {
  return memo_slots(dev, kMemoTgpu16 + elem * 2 + wide,
                    [&] { return fa_tgpu16::occupancy_s1(elem, wide); });
}

// The dynamic LDS the S = 2 launch reserves (and never uses) so that at most
// kTgpuS2Resident of its workgroups share a CU.  Measured r05
// (profiles/r05_ab_lib_tgpu_s2.jsonl, same process) on the kernel before its
// S = 4 riders (100 VGPRs, five per CU): three per CU 3-4 % faster than five,
// two 10 % slower (a reservation of exactly a third of the CU's LDS admitted
// only two: the allocation rounds up).  With the riders' paths it holds 130
// VGPRs, three per CU by itself; the reservation keeps the measured count if
// that changes.  The default reduce's 8-client kernels capped the same way
// ran 20-25 % slower (r05_ab_lib_occupancy_cap.jsonl).  0 when the device
// cannot say.
#ifndef FA_TGPU_S2_RESIDENT
#define FA_TGPU_S2_RESIDENT 3
#endif
constexpr int kTgpuS2Resident = FA_TGPU_S2_RESIDENT;
size_t tgpu_s2_lds(int dev) {
  return (size_t)dev_memo(dev, kMemoS2Lds, [&]() -> int64_t {
    int per_cu = 0;
    if (hipDeviceGetAttribute(&per_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) !=
        hipSuccess)
      per_cu = 0;
    // per_cu / (resident + 1/2): the allocation granularity may round the
    // request up, and per_cu / resident exactly would then admit one fewer
    return per_cu > 0 ? (2 * (int64_t)per_cu / (2 * kTgpuS2Resident + 1)) & ~(int64_t)1023 : 0;
  });
}

hipError_t launch_chain(const ReduceArgs& a, int ntiles, int vec_u, hipStream_t st) {
  const bool deep = a.n_total >= 256;
  const bool w = a.flags & 0x100u;
  if (vec_u == 1) return launch_chain_ub<1, 8>(a, ntiles, deep, w, st);
  if (vec_u == 4) return launch_chain_ub<4, 8>(a, ntiles, deep, w, st);
  if (w || a.n < 16) return launch_chain_ub<2, 8>(a, ntiles, deep, w, st);
  return launch_chain_ub<2, 16>(a, ntiles, deep, w, st);
}


// batch, pipe: the launch rules' choice (fa_host::select_launch)
hipError_t launch_reduce(const ReduceArgs& a, int ntiles, int vec_u, hipStream_t st, int b,
                         int pipe) {
  // DEEP (n >= 256): cascade levels 2-3 and the constant-space table loads.
  // Weighted reductions take the mean's 16-client batches too since the
  // batch's weights are read once up front (r02 sweep, same box: weighted
  // U2xB16 140.5 us vs U2xB8 143.3 us, unweighted 143.0 us).
  const bool deep = a.n >= 256;
  const bool w = a.flags & 0x100u;  // internal: weighted
  switch (vec_u) {
    case 1: return b == 16 ? launch_u<1, 16>(a, ntiles, deep, w, 0, st)
                           : launch_u<1, 8>(a, ntiles, deep, w, 0, st);
    case 4: return launch_u<4, 8>(a, ntiles, deep, w, 0, st);
    default: return b == 16 ? launch_u<2, 16>(a, ntiles, deep, w, pipe, st)
                            : launch_u<2, 8>(a, ntiles, deep, w, pipe, st);
  }
}

// Stateless-API plan cache, keyed by device + layout.
std::mutex g_cache_mu;
std::map<std::string, fa_plan*> g_cache;

int cached_plan(const fa_seg* s32, int n32, int64_t numel32, const fa_seg* s64, int n64,
                int64_t numel64, fa_plan** out) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::string key((const char*)&dev, sizeof dev);
  key.append((const char*)&numel32, sizeof numel32);
  key.append((const char*)&numel64, sizeof numel64);
  key.append((const char*)&n32, sizeof n32);
  if (n32 > 0) key.append((const char*)s32, sizeof(fa_seg) * n32);
  if (n64 > 0) key.append((const char*)s64, sizeof(fa_seg) * n64);
  std::lock_guard<std::mutex> lk(g_cache_mu);
  auto it = g_cache.find(key);
  if (it != g_cache.end()) { *out = it->second; return FA_OK; }
  fa_plan* p = nullptr;
  int rc = fa_plan_create(s32, n32, numel32, s64, n64, numel64, 0, 0, &p);
  if (rc) return rc;
  g_cache[key] = p;
  *out = p;
  return FA_OK;
}

}  // namespace

// =================================================================== ABI ==
namespace {
// Client pointer tables (N > kInline) come from a private stream-ordered pool
// whose freed blocks are reused only by the stream that freed them: cross-
// stream reuse (opportunistic or internal-dependency) is switched off, so a
// table still read by a kernel on one stream can never be handed to another
// stream (the executor in fedcomm.hip drives two).  The loopback test of the
// multi-rank rounds saw payload corruption with cross-stream frees on the
// default pool (tests/loopback/loopccl.hip).
hipError_t table_alloc(void** p, size_t bytes, hipStream_t st) {
  static std::mutex mu;
  static std::map<int, hipMemPool_t> pools;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  hipMemPool_t pool = nullptr;
  {
    std::lock_guard<std::mutex> lk(mu);
    auto it = pools.find(dev);
    if (it != pools.end()) {
      pool = it->second;
    } else {
      hipMemPoolProps props{};
      props.allocType = hipMemAllocationTypePinned;
      props.location.type = hipMemLocationTypeDevice;
      props.location.id = dev;
      e = hipMemPoolCreate(&pool, &props);
      if (e != hipSuccess) return e;
      int off = 0;
      for (hipMemPoolAttr a : {hipMemPoolReuseFollowEventDependencies,
                               hipMemPoolReuseAllowOpportunistic,
                               hipMemPoolReuseAllowInternalDependencies})
        if ((e = hipMemPoolSetAttribute(pool, a, &off)) != hipSuccess) return e;
      uint64_t keep = UINT64_MAX;  // keep freed blocks for the next round
      if ((e = hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep)) != hipSuccess)
        return e;
      pools[dev] = pool;
    }
  }
  return hipMallocFromPoolAsync(p, bytes, pool, st);
}

// A caller-owned pointer table (fa_reduce_tab) is written by kernels whose
// arguments carry the words by value: no host memcpy, no allocation, so the
// call can be captured into a graph and replayed (the table's contents are
// the kernel arguments, frozen at capture).
constexpr int kFillWords = 400;
struct FillArgs {
  uint64_t* dst;
  int count;
  uint64_t w[kFillWords];
};
__global__ void table_fill_kernel(FillArgs a) {
  for (int i = threadIdx.x; i < a.count; i += blockDim.x) a.dst[i] = a.w[i];
}
hipError_t table_fill(void* dst, const std::vector<char>& host, hipStream_t st) {
  const size_t words = (host.size() + 7) / 8;
  for (size_t w0 = 0; w0 < words; w0 += kFillWords) {
    FillArgs f;
    memset(&f, 0, sizeof f);
    f.dst = (uint64_t*)dst + w0;
    f.count = (int)std::min<size_t>(kFillWords, words - w0);
    memcpy(f.w, host.data() + w0 * 8, std::min<size_t>(f.count * 8, host.size() - w0 * 8));
    hipLaunchKernelGGL(table_fill_kernel, dim3(1), dim3(256), 0, st, f);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
}  // namespace

namespace {
// Free a plan's device tables and the plan itself (fa_plan_destroy, and
// PlanPtr below): the first hipFree error; every table is freed all the same.
hipError_t plan_free(fa_plan* p) {
  hipError_t first = hipSuccess;
  std::vector<void*> tabs = {p->d_fac, p->d_tiles, p->d_tiles_alt, p->d_sidx};
  tabs.insert(tabs.end(), p->d_bal.begin(), p->d_bal.end());
  for (void* d : tabs) {
    const hipError_t e = d ? hipFree(d) : hipSuccess;
    if (first == hipSuccess) first = e;
  }
  delete p;
  return first;
}
// A plan under construction: every error path frees whatever was uploaded;
// a create path releases it into *out only on success.
struct PlanDelete {
  void operator()(fa_plan* p) const { (void)plan_free(p); }
};
using PlanPtr = std::unique_ptr<fa_plan, PlanDelete>;

template <class T>
hipError_t upload(T** d, const std::vector<T>& h) {
  if (h.empty()) return hipSuccess;
  const hipError_t e = hipMalloc(d, h.size() * sizeof(T));
  return e != hipSuccess ? e : hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
}

// Upload a CPU-order plan's device tables (fa_host::plan_tables: main +
// optional alt, the shared scalar index, the balanced tables).
hipError_t upload_tables(fa_plan* p, const std::vector<Tile>& tiles,
                         const std::vector<Tile>& alt) {
  const fa_host::HostTables h =
      fa_host::plan_tables(tiles, alt, p->vec_u, p->flags, p->device, kernel_slots);
  p->nt = (int)h.main.size();
  p->ns = h.ns_main;
  p->nt_alt = (int)h.alt.size();
  p->ns_alt = h.ns_alt;
  p->sidx_alt_off = h.sidx_alt_off;
  hipError_t e = upload(&p->d_tiles, h.main);
  if (e == hipSuccess) e = upload(&p->d_tiles_alt, h.alt);
  if (e == hipSuccess) e = upload(&p->d_sidx, h.sidx);
  for (const fa_host::HostTables::Bal& b : h.bal) {
    if (e != hipSuccess) break;
    Tile* d = nullptr;
    e = upload(&d, b.tiles);
    if (!d) break;
    p->bal.push_back({b.u, b.slots, b.batch, (int)b.tiles.size(), b.alt});
    p->d_bal.push_back(d);
  }
  return e;
}

// What a plan entry point asks for: every segment-list entry fills one and
// hands it to plan_from_segs.
struct PlanSpec {
  const char* who;         // the entry's name in the messages
  const char* flags_hint;  // the tail of its unknown-flag message
  const fa_seg* seg32; int nseg32; int64_t f32_numel;  // the floating bucket
  const fa_seg* seg64; int nseg64; int64_t i64_numel;  // the int64 bucket
  int tile_elems;  // the CPU order only (0 from the _order entries)
  unsigned flags;
  int n, order;    // the _order entries only
  int elem, out_elem;
};

// The result bucket's type is the clients', or FA_ELEM_F32 over 16-bit
// clients (a mixed plan: the fp32 master global).
int check_elems(const char* who, int elem, int out_elem) {
  if ((elem == FA_ELEM_F16 || elem == FA_ELEM_BF16) &&
      (out_elem == elem || out_elem == FA_ELEM_F32))
    return FA_OK;
  return set_err(FA_E_INVAL, "%s: out_elem must equal elem, or be FA_ELEM_F32 over FA_ELEM_F16 / "
                             "FA_ELEM_BF16 clients (got elem %d, out_elem %d)", who, elem, out_elem);
}

// The CPU-order body (fa_plan_create, _elem, _elem_out).  A 16-bit plan (elem
// FA_ELEM_F16 / FA_ELEM_BF16) holds the plain table only, cut at 16-B
// vectors of 8 elements; a mixed plan (out_elem FA_ELEM_F32 over 16-bit
// clients) is that table, reduced by the wide-store instances of the 16-bit
// kernels into an fp32 bucket at the same element offsets and broadcast by
// the narrowing kernel.
int plan_create_cpu(const PlanSpec& s, fa_plan** out) {
  if (!out) return set_err(FA_E_INVAL, "%s: out is NULL", s.who);
  *out = nullptr;
  fa_host::Layout l;
  int rc = fa_host::parse_layout(s.who, s.flags_hint, fa_host::kCheckSizes | fa_host::kCheckTile,
                                 s.seg32, s.nseg32, s.f32_numel, s.seg64, s.nseg64, s.i64_numel,
                                 s.tile_elems, s.flags, s.elem, &l);
  if (rc) return rc;
  const bool h16 = s.elem != FA_ELEM_F32;
  PlanPtr p(new fa_plan());
  p->family = h16 ? FaFamily::kH16 : FaFamily::kDefault;
  p->elem = s.elem;
  p->out_elem = s.out_elem;
  p->info = l.info;
  p->vec_u = l.info.tile_elems / (h16 ? fa_h16::kTile : 4 * kBlock);
  // a 16-bit plan: the plain table is the one launched
  p->flags = h16 ? s.flags | FA_PLAN_TUNE_NO_BALANCE : s.flags;
  p->flat_bcast = fa_host::flat_bcast_ok(s.flags, l, s.elem, s.out_elem);
  std::vector<Tile> tiles, alt;
  rc = fa_host::build_tiles(l.s32, l.s64, l.info.tile_elems, s.flags, &tiles, &p->info, l.valign);
  if (rc) return rc;
  set_kinds(p.get(), tiles);
  if (l.autosel) {
    fa_plan_info ia{};
    rc = fa_host::build_tiles(l.s32, l.s64, 4 * kBlock, s.flags, &alt, &ia);
    if (rc) return rc;
  }
  hipError_t e = hipGetDevice(&p->device);
  if (e == hipSuccess) e = upload_tables(p.get(), tiles, alt);
  if (e != hipSuccess)
    return set_err(FA_E_HIP, "%s: %s", h16 ? "fa_plan_create_elem" : "fa_plan_create",
                   hipGetErrorString(e));
  *out = p.release();
  return FA_OK;
}

// The torch-GPU-order body (fa_plan_create_order, _order_elem,
// _order_elem_out).  Two arms, each with the checks of the entry it came
// from in that entry's order.  fp32: order, n, the segments (no size or tile
// check; 1024-float tiles), then the device is asked for tgpu_kernel<0>'s
// slots.  16-bit: the table fa_plan_build_order_host_elem returns for the
// clients' type (fa_host::plan_order_elem: order, n, elem, sizes, segments),
// with a result bucket of that type or (out_elem FA_ELEM_F32) an fp32 one at
// the same element offsets; the slots of its S = 1 kernel are asked before
// those checks, and only for an element type that has a kernel.
int plan_create_tgpu(const PlanSpec& s, fa_plan** out) {
  int rc = fa_host::check_flags(s.who, s.flags);
  if (rc) return rc;
  if (!out) return set_err(FA_E_INVAL, "%s: out is NULL", s.who);
  *out = nullptr;
  const bool h16 = s.elem != FA_ELEM_F32;
  const bool balance = !(s.flags & FA_PLAN_TUNE_NO_BALANCE);
  fa_host::Layout l;
  fa_host::TgpuTables t;
  int dev = 0;
  hipError_t e;
  if (h16) {
    e = hipGetDevice(&dev);
    const bool known = s.elem == FA_ELEM_F16 || s.elem == FA_ELEM_BF16;
    const int slots = e == hipSuccess && known && balance
                          ? tgpu16_slots(dev, s.elem, s.out_elem != s.elem)
                          : 0;
    rc = fa_host::plan_order_elem(s.who, s.seg32, s.nseg32, s.f32_numel, s.seg64, s.nseg64,
                                  s.i64_numel, s.n, s.order, s.flags, s.elem, slots, &l, &t);
  } else {
    if (s.order != FA_ORDER_TORCH_GPU)
      return set_err(FA_E_INVAL, "%s: order %d", s.who, s.order);
    if (s.n < 2 || s.n > FA_MAX_CLIENTS)
      return set_err(FA_E_RANGE, "%s: n=%d outside 2..%d", s.who, s.n, FA_MAX_CLIENTS);
    rc = fa_host::parse_layout(s.who, "", 0, s.seg32, s.nseg32, s.f32_numel, s.seg64, s.nseg64,
                               s.i64_numel, 4 * kBlock, s.flags, FA_ELEM_F32, &l);
    if (rc) return rc;
    e = hipGetDevice(&dev);
    const int slots =
        e == hipSuccess && balance ? tgpu_slots(dev, fa_host::tgpu_batch_for(s.n)) : 0;
    rc = fa_host::plan_tgpu(l.s32, l.s64, s.n, s.flags, slots, &t);
  }
  if (rc) return rc;
  PlanPtr p(new fa_plan());
  p->family = h16 ? FaFamily::kTgpu16 : FaFamily::kTgpu;
  for (int g = 0; g < 6; ++g) p->tg_lo[g] = t.lo[g];
  p->info = l.info;
  p->info.ntiles = (int32_t)t.tiles.size();
  p->info.ntiles_tail = (int32_t)t.tiles.size();
  p->flags = s.flags;
  p->elem = s.elem;
  p->out_elem = s.out_elem;
  p->flat_bcast = fa_host::flat_bcast_ok(s.flags, l, s.elem, s.out_elem);
  p->order_n = s.n;
  set_kinds(p.get(), t.tiles);
  p->device = dev;
  if (h16) {
    // (no LDS reservation on the S = 2 launch: tgpu_s2_lds was measured on
    // the fp32 instance only)
    p->vec_u = 1;
  } else {
    p->tgpu_batch = fa_host::tgpu_batch_for(s.n);
    if (e == hipSuccess) p->tgpu_s2_lds = tgpu_s2_lds(dev);
  }
  if (e == hipSuccess) e = upload(&p->d_tiles, t.tiles);
  if (e == hipSuccess) e = upload(&p->d_fac, t.fac);
  if (e != hipSuccess) return set_err(FA_E_HIP, "%s: %s", s.who, hipGetErrorString(e));
  *out = p.release();
  return FA_OK;
}

// The forwarding rules of the six segment-list entries, in one place.  A
// call is named, in every message, by what it asks for and not by the symbol
// it came through: FA_ELEM_F32 drops "_elem", out_elem == elem drops "_out",
// FA_ORDER_TORCH_CPU drops "_order" — an _elem entry given FA_ELEM_F32 is
// the plain entry, an _elem_out entry with out_elem == elem the _elem entry,
// an _order* entry with the CPU order the entry without the order (DESIGN
// §3.1 has the table).  One trace of the symbol stays: fa_plan_create_order
// checks the flag bits under its own name before it forwards the CPU order
// (`order_entry`: the call came through an _order* symbol).
int plan_from_segs(PlanSpec s, bool order_entry, fa_plan** out) {
  static const char* const kWho[2][3] = {
      {"fa_plan_create", "fa_plan_create_elem", "fa_plan_create_elem_out"},
      {"fa_plan_create_order", "fa_plan_create_order_elem", "fa_plan_create_order_elem_out"}};
  const bool tgpu = s.order != FA_ORDER_TORCH_CPU;
  const bool h16 = s.elem != FA_ELEM_F32, mixed = s.out_elem != s.elem;
  const bool plain = !h16 && !mixed;
  if (order_entry && plain) {
    const int rc = fa_host::check_flags(kWho[1][0], s.flags);
    if (rc) return rc;
  }
  s.who = kWho[tgpu][mixed ? 2 : h16];
  s.flags_hint = plain && !tgpu ? " (removed tuning flags?)" : "";
  if (mixed) {
    if (!out) return set_err(FA_E_INVAL, "%s: out is NULL", s.who);
    *out = nullptr;
    const int rc = check_elems(s.who, s.elem, s.out_elem);
    if (rc) return rc;
  }
  return tgpu ? plan_create_tgpu(s, out) : plan_create_cpu(s, out);
}
}  // namespace

extern "C" {

const char* fa_version(void) { return FA_VERSION_STR; }
const char* fa_last_error(void) { return g_last_error.c_str(); }

int fa_plan_create(const fa_seg* seg32, int nseg32, int64_t f32_numel, const fa_seg* seg64,
                   int nseg64, int64_t i64_numel, int tile_elems, unsigned flags,
                   fa_plan** out) {
  return plan_from_segs({nullptr, nullptr, seg32, nseg32, f32_numel, seg64, nseg64, i64_numel,
                         tile_elems, flags, 0, FA_ORDER_TORCH_CPU, FA_ELEM_F32, FA_ELEM_F32},
                        false, out);
}

int fa_plan_create_elem(const fa_seg* seg32, int nseg32, int64_t f32_numel, const fa_seg* seg64,
                        int nseg64, int64_t i64_numel, int tile_elems, unsigned flags, int elem,
                        fa_plan** out) {
  return plan_from_segs({nullptr, nullptr, seg32, nseg32, f32_numel, seg64, nseg64, i64_numel,
                         tile_elems, flags, 0, FA_ORDER_TORCH_CPU, elem, elem},
                        false, out);
}

int fa_plan_create_elem_out(const fa_seg* seg32, int nseg32, int64_t f32_numel,
                            const fa_seg* seg64, int nseg64, int64_t i64_numel, int tile_elems,
                            unsigned flags, int elem, int out_elem, fa_plan** out) {
  return plan_from_segs({nullptr, nullptr, seg32, nseg32, f32_numel, seg64, nseg64, i64_numel,
                         tile_elems, flags, 0, FA_ORDER_TORCH_CPU, elem, out_elem},
                        false, out);
}

int fa_plan_create_order(const fa_seg* seg32, int nseg32, int64_t f32_numel, const fa_seg* seg64,
                         int nseg64, int64_t i64_numel, int n, int order, unsigned flags,
                         fa_plan** out) {
  return plan_from_segs({nullptr, nullptr, seg32, nseg32, f32_numel, seg64, nseg64, i64_numel, 0,
                         flags, n, order, FA_ELEM_F32, FA_ELEM_F32},
                        true, out);
}

int fa_plan_create_order_elem(const fa_seg* seg32, int nseg32, int64_t f32_numel,
                              const fa_seg* seg64, int nseg64, int64_t i64_numel, int n, int order,
                              unsigned flags, int elem, fa_plan** out) {
  return plan_from_segs({nullptr, nullptr, seg32, nseg32, f32_numel, seg64, nseg64, i64_numel, 0,
                         flags, n, order, elem, elem},
                        true, out);
}

int fa_plan_create_order_elem_out(const fa_seg* seg32, int nseg32, int64_t f32_numel,
                                  const fa_seg* seg64, int nseg64, int64_t i64_numel, int n,
                                  int order, unsigned flags, int elem, int out_elem,
                                  fa_plan** out) {
  return plan_from_segs({nullptr, nullptr, seg32, nseg32, f32_numel, seg64, nseg64, i64_numel, 0,
                         flags, n, order, elem, out_elem},
                        true, out);
}

int fa_plan_elem(const fa_plan* plan) {
  if (!plan) return set_err(FA_E_INVAL, "fa_plan_elem: plan is NULL");
  return plan->elem;
}

int fa_plan_out_elem(const fa_plan* plan) {
  if (!plan) return set_err(FA_E_INVAL, "fa_plan_out_elem: plan is NULL");
  return plan->out_elem;
}

namespace {
// One body behind fa_plan_create_from_tiles and ..._from_tiles_elem (`who`,
// in the messages).  A 16-bit or mixed subset plan is cut from
// fa_plan_build_host_elem's table: vectors of 8 elements, tiles of 2048 or
// 4096, launched by the 16-bit kernels as a segment plan's table is; it
// covers no bucket (flat_bcast stays false), so fa_reduce refuses its
// broadcast.  Every refusal returns before the first device call.
int plan_from_tiles(const char* who, const fa_tile_desc* tiles, int ntiles, int64_t f32_numel,
                    int64_t i64_numel, int tile_elems, unsigned flags, int elem, int out_elem,
                    fa_plan** out) {
  if (!out) return set_err(FA_E_INVAL, "%s: out is NULL", who);
  *out = nullptr;
  int rc = fa_host::check_flags(who, flags);
  if (rc) return rc;
  if (ntiles < 0 || (ntiles > 0 && !tiles)) return set_err(FA_E_INVAL, "%s: bad tile array", who);
  const bool h16 = elem != FA_ELEM_F32;
  const int valign = h16 ? fa_h16::kVec : 4;
  if (h16) {
    if (tile_elems == 0) tile_elems = fa_h16::kDefaultU * fa_h16::kTile;
    if (tile_elems != fa_h16::kTile && tile_elems != 2 * fa_h16::kTile)
      return set_err(FA_E_INVAL, "%s: a 16-bit plan's tile_elems must be 2048 or 4096 (got %d)",
                     who, tile_elems);
  } else {
    if (tile_elems == 0) tile_elems = 4 * kBlock * kDefaultU;
    if (tile_elems != 4 * kBlock && tile_elems != 8 * kBlock && tile_elems != 16 * kBlock)
      return set_err(FA_E_INVAL, "tile_elems must be 1024, 2048 or 4096 (got %d)", tile_elems);
  }
  fa_plan_info in{};
  in.f32_numel = f32_numel;
  in.i64_numel = i64_numel;
  in.tile_elems = tile_elems;
  std::vector<Tile> vec, sc;
  for (int i = 0; i < ntiles; ++i) {
    const fa_tile_desc& d = tiles[i];
    const bool is64 = d.kind >= K_I64_CASC;
    const int64_t lim = is64 ? i64_numel : f32_numel;
    if (d.kind < K_F32_VEC || d.kind > K_I64_INNER || d.count < 1 || d.start < 0 ||
        d.start + d.count > lim)
      return set_err(FA_E_INVAL, "tile %d: kind %d [%lld,+%d) invalid", i, d.kind,
                     (long long)d.start, d.count);
    if (d.kind == K_F32_VEC) {
      if (d.start % valign || d.count % valign || d.count > tile_elems)
        return set_err(FA_E_INVAL, "tile %d: vector tile must be %d-aligned and <= %d", i, valign,
                       tile_elems);
      vec.push_back(Tile{d.start, d.count, d.kind});
      in.cascade_elems += d.count;
    } else {
      if (d.count > kBlock) return set_err(FA_E_INVAL, "tile %d: scalar tile > %d", i, kBlock);
      sc.push_back(Tile{d.start, d.count, d.kind});
      if (!is64) in.tail_elems += d.count;
    }
  }
  std::vector<Tile> t(sc);
  t.insert(t.end(), vec.begin(), vec.end());
  rc = fa_host::check_disjoint(t, who);
  if (rc) return rc;
  in.ntiles = (int32_t)t.size();
  in.ntiles_cascade = (int32_t)vec.size();
  in.ntiles_tail = (int32_t)sc.size();
  PlanPtr p(new fa_plan());
  p->family = h16 ? FaFamily::kH16 : FaFamily::kDefault;
  p->info = in;
  p->elem = elem;
  p->out_elem = out_elem;
  p->vec_u = tile_elems / (h16 ? fa_h16::kTile : 4 * kBlock);
  p->flags = flags | FA_PLAN_TUNE_NO_BALANCE;  // the caller's tiles are the ones launched
  set_kinds(p.get(), t);
  hipError_t e = hipGetDevice(&p->device);
  if (e == hipSuccess) e = upload_tables(p.get(), t, {});
  if (e != hipSuccess) return set_err(FA_E_HIP, "%s: %s", who, hipGetErrorString(e));
  *out = p.release();
  return FA_OK;
}
}  // namespace

int fa_plan_create_from_tiles(const fa_tile_desc* tiles, int ntiles, int64_t f32_numel,
                              int64_t i64_numel, int tile_elems, unsigned flags,
                              fa_plan** out) {
  return plan_from_tiles("fa_plan_create_from_tiles", tiles, ntiles, f32_numel, i64_numel,
                         tile_elems, flags, FA_ELEM_F32, FA_ELEM_F32, out);
}

int fa_plan_create_from_tiles_elem(const fa_tile_desc* tiles, int ntiles, int64_t f32_numel,
                                   int64_t i64_numel, int tile_elems, unsigned flags, int elem,
                                   int out_elem, fa_plan** out) {
  if (elem == FA_ELEM_F32 && out_elem == FA_ELEM_F32)
    return fa_plan_create_from_tiles(tiles, ntiles, f32_numel, i64_numel, tile_elems, flags, out);
  const char* who = "fa_plan_create_from_tiles_elem";
  if (!out) return set_err(FA_E_INVAL, "%s: out is NULL", who);
  *out = nullptr;
  const int rc = check_elems(who, elem, out_elem);
  if (rc) return rc;
  return plan_from_tiles(who, tiles, ntiles, f32_numel, i64_numel, tile_elems, flags, elem, out_elem,
                         out);
}

int fa_plan_destroy(fa_plan* plan) {
  if (!plan) return FA_OK;
  const hipError_t e = plan_free(plan);
  if (e != hipSuccess) return set_err(FA_E_HIP, "fa_plan_destroy: hipFree: %s", hipGetErrorString(e));
  return FA_OK;
}

int fa_plan_get_info(const fa_plan* plan, fa_plan_info* info) {
  if (!plan || !info) return set_err(FA_E_INVAL, "fa_plan_get_info: NULL argument");
  *info = plan->info;
  return FA_OK;
}

namespace {
// The round's broadcast launch (after the reduce, over the arguments the
// reduce used): the flat copy in client groups on gap-padded plans
// (bcast_flat2_kernel), client groups per tile through the tile table
// otherwise (bcast_group2_kernel).  Scalar pointer loads, client groups of
// <= kBcastGroupMax = 24, 1024-float parts, destination stores sc1 nt.
// Measured inside the round, same process, after the reduce's result stores
// became sc1 (tools/archive/exp_round2.py, profiles/r04_exp_round2_bcast_forms.jsonl):
// groups of <= 24 vs <= 10 cfg2 283.7 / 282.4 vs 284.9 / 285.0 us, cfg5 (24
// slots: one group vs three) 350.0 vs 363.5 us, the small layouts equal; and
// one source fetch instead of one per group (PMC: broadcast traffic 1.0012
// vs 1.0486 x algorithmic, profiles/r04_round_pmc_round*.json).
extern "C++" template <int G>
void launch_bcast2(const fa_plan* plan, ReduceArgs& a, int ntiles, uint32_t groups,
                   uint32_t gsize, hipStream_t st) {
  if (plan->flat_bcast) {
    // (a 16-bit bucket is copied as numel / 2 floats: the same bytes)
    const int64_t f = plan->has32 ? plan->info.f32_numel / (plan->elem == FA_ELEM_F32 ? 1 : 2) : 0;
    const int64_t i = plan->has64 ? plan->info.i64_numel : 0;
    const int64_t parts = f > 0 ? std::max<int64_t>(1, (f / 4 + kBlock - 1) / kBlock) : 0;
    const int64_t np = parts + (i > 0 ? 1 : 0);
    if (np == 0) return;
    hipLaunchKernelGGL((bcast_flat2_kernel<G>), dim3((unsigned)(np * groups)), dim3(kBlock), 0,
                       st, a, (uint32_t)parts, groups, gsize, f, i);
  } else if (ntiles > 0) {
    hipLaunchKernelGGL((bcast_group2_kernel<G>), dim3((unsigned)ntiles * groups), dim3(kBlock), 0,
                       st, a, groups, gsize);
  }
}

hipError_t launch_bcast(const fa_plan* plan, ReduceArgs& a, int n, int ntiles, hipStream_t st) {
  a.flags |= FA_F_BCAST;
  if (n <= 0) return hipSuccess;
  if (plan->elem != plan->out_elem)  // a mixed plan: fp32 result -> 16-bit clients
    return fa_h16::bcast_narrow(a, n, plan->elem, plan->has32 ? plan->info.f32_numel : 0,
                                plan->has64 ? plan->info.i64_numel : 0, st);
  const uint32_t groups = (uint32_t)((n + kBcastGroupMax - 1) / kBcastGroupMax);
  const uint32_t gsize = (uint32_t)((n + groups - 1) / groups);
  // grids stay below 2^32 blocks: n clients of >= 4 KB parts would outgrow
  // any GPU's memory long before
  const int64_t units = plan->flat_bcast ? (plan->info.f32_numel / 1024 + 2) : ntiles;
  if (units * (int64_t)groups > (int64_t)UINT32_MAX) return hipErrorInvalidValue;
  if (gsize <= 8) launch_bcast2<8>(plan, a, ntiles, groups, gsize, st);
  else if (gsize <= 16) launch_bcast2<16>(plan, a, ntiles, groups, gsize, st);
  else launch_bcast2<24>(plan, a, ntiles, groups, gsize, st);
  return hipGetLastError();
}
}  // namespace

int fa_plan_launch_shape(const fa_plan* plan, int n, int weighted, int* ntiles, int* slots) {
  if (!plan || !ntiles || !slots || n < 1)
    return set_err(FA_E_INVAL, "fa_plan_launch_shape: bad arguments");
  *slots = 0;
  switch (plan->family) {
    case FaFamily::kTgpu:
    case FaFamily::kTgpu16: *ntiles = plan->info.ntiles; break;
    case FaFamily::kH16: *ntiles = plan->nt; break;  // one table, launched as it is
    case FaFamily::kDefault: {
      const fa_host::Launch L = fa_host::select_launch(*plan, n, weighted != 0, kernel_slots);
      *ntiles = L.nt;
      *slots = L.slots ? L.slots
                       : fa_host::call_slots(plan->device, n, L.vec_u, weighted != 0,
                                             plan->flags & ~FA_PLAN_TUNE_NO_BALANCE, kernel_slots);
    }
  }
  return FA_OK;
}

int fa_plan_launch_form(const fa_plan* plan, int n, int weighted, int* tile_elems, int* batch,
                        int* pipe) {
  if (!plan || !tile_elems || !batch || !pipe || n < 1)
    return set_err(FA_E_INVAL, "fa_plan_launch_form: bad arguments");
  switch (plan->family) {
    case FaFamily::kTgpu:
    case FaFamily::kTgpu16: *tile_elems = *batch = *pipe = 0; break;
    case FaFamily::kH16:  // the client loop, one client per step
      *tile_elems = plan->info.tile_elems;
      *batch = *pipe = 1;
      break;
    case FaFamily::kDefault: {
      const fa_host::Launch L = fa_host::select_launch(*plan, n, weighted != 0, kernel_slots);
      *tile_elems = 4 * kBlock * L.vec_u;
      *batch = L.batch;
      *pipe = L.pipe;
    }
  }
  return FA_OK;
}

size_t fa_table_bytes(int n) { return n > kInline ? ((size_t)n * 20 + 7) / 8 * 8 : 0; }

int fa_reduce(const fa_plan* plan, const float* const* c32, const int64_t* const* c64, int n,
              const float* weights, float* out32, int64_t* out64, unsigned flags,
              void* stream) {
  return fa_reduce_tab(plan, c32, c64, n, weights, nullptr, out32, out64, flags, stream);
}

namespace {
// A call's client pointers and weights.  n <= kInline: copied into the
// kernel arguments, no allocation and no HIP call.  More: a device table
// [n fp32 ptrs][n int64 ptrs][n weights] — the caller's (ctable: written by
// kernels, no memcpy), or a stream-ordered allocation that done() / the
// scope's end frees on the stream.  c32 / c64 NULL: that bucket is not read.
struct ClientTable {
  hipStream_t st;
  void* owned = nullptr;

  hipError_t fill(ReduceArgs& a, const float* const* c32, const int64_t* const* c64, int n,
                  const float* weights, void* ctable) {
    if (n <= kInline) {
      for (int i = 0; i < n; ++i) {
        if (c32) a.c32[i] = c32[i];
        if (c64) a.c64[i] = c64[i];
        if (weights) a.w[i] = weights[i];
      }
      return hipSuccess;
    }
    std::vector<char> host((size_t)n * 20);
    const void** h32 = (const void**)host.data();
    const void** h64 = h32 + n;
    float* hw = (float*)(h64 + n);
    for (int i = 0; i < n; ++i) {
      h32[i] = c32 ? (const void*)c32[i] : nullptr;
      h64[i] = c64 ? (const void*)c64[i] : nullptr;
      hw[i] = weights ? weights[i] : 0.f;
    }
    hipError_t e;
    if (ctable) {
      e = table_fill(ctable, host, st);
    } else {
      e = table_alloc(&owned, host.size(), st);
      // `host` dies at return: this relies on the runtime staging a pageable
      // source before hipMemcpyAsync returns (not so for a
      // caller's table, which kernels fill)
      if (e == hipSuccess)
        e = hipMemcpyAsync(owned, host.data(), host.size(), hipMemcpyHostToDevice, st);
    }
    const void** tab = (const void**)(ctable ? ctable : owned);
    a.tab32 = (const float* const*)tab;
    a.tab64 = (const int64_t* const*)(tab + n);
    a.tabw = (const float*)(tab + 2 * n);
    return e;
  }
  // the call's outcome: `e`, or the free's error when the launches went well
  hipError_t done(hipError_t e) {
    if (owned) {
      const hipError_t e2 = hipFreeAsync(owned, st);
      owned = nullptr;
      if (e == hipSuccess) e = e2;
    }
    return e;
  }
  ~ClientTable() { (void)done(hipSuccess); }
};

// the broadcast alone (the reference's initial sync, train_fedavg.py:
// 244-250, and :148-149 without the reduce): out32/out64 -> every client
hipError_t run_bcast_only(const fa_plan* plan, ReduceArgs& a, int n, hipStream_t st) {
  const int nt = plan->tgpu() ? plan->info.ntiles : plan->nt;
  a.ntiles = nt;
  a.sidx = plan->d_sidx;
  return launch_bcast(plan, a, n, nt, st);
}

// A torch-GPU-order plan: one launch per row-split group of its table
// (`launch(g, cnt)`, inlined: the per-round host path), then the broadcast
// as its own launch over the whole table — client groups per tile (as the
// default order's split broadcast); on a 16-bit plan the flat byte copy of
// the result bucket (fa_reduce_tab has refused one without coverage) or, with
// an fp32 result bucket, the narrowing broadcast.
extern "C++" template <class LaunchGroup>
hipError_t run_groups(const fa_plan* plan, ReduceArgs& a, int n, bool bcast, hipStream_t st,
                      LaunchGroup launch) {
  hipError_t e = hipSuccess;
  for (int g = 0; g < 5 && e == hipSuccess; ++g) {
    const int lo = plan->tg_lo[g], cnt = plan->tg_lo[g + 1] - lo;
    if (cnt == 0) continue;
    a.tiles = plan->d_tiles + lo;
    a.tfac = plan->d_fac + lo;
    a.ntiles = cnt;
    e = launch(g, cnt);
  }
  if (e == hipSuccess && bcast && plan->tg_lo[5] > 0) {
    a.tiles = plan->d_tiles;
    a.ntiles = plan->tg_lo[5];
    e = launch_bcast(plan, a, n, a.ntiles, st);
  }
  return e;
}

hipError_t run_tgpu(const fa_plan* plan, ReduceArgs& a, int n, bool bcast, hipStream_t st) {
  return run_groups(plan, a, n, bcast, st, [&](int g, int cnt) {
    switch (g) {
      case 0:
        // the client loop on full tiles at every N (r05,
        // profiles/r05_ab_lib_tgpu_client_loop.jsonl)
        if (plan->tgpu_batch == 8)
          hipLaunchKernelGGL((tgpu_kernel<0, 8, 1>), dim3(cnt), dim3(kBlock), 0, st, a);
        else
          hipLaunchKernelGGL((tgpu_kernel<0, 16, 1>), dim3(cnt), dim3(kBlock), 0, st, a);
        break;
      case 1:
        hipLaunchKernelGGL(tgpu_kernel<1>, dim3(cnt), dim3(kBlock), plan->tgpu_s2_lds, st, a);
        break;
      case 2: hipLaunchKernelGGL(tgpu_kernel<2>, dim3(cnt), dim3(kBlock), 0, st, a); break;
      case 3: hipLaunchKernelGGL(tgpu_kernel<3>, dim3(cnt), dim3(kBlock), 0, st, a); break;
      default: hipLaunchKernelGGL(tgpu_kernel<4>, dim3(cnt), dim3(kBlock), 0, st, a); break;
    }
    return hipGetLastError();
  });
}

// fedagg_tgpu16.hip's kernels; with an fp32 result bucket
// (fa_plan_create_order_elem_out) their wide-store instances
hipError_t run_tgpu16(const fa_plan* plan, ReduceArgs& a, int n, bool bcast, hipStream_t st) {
  return run_groups(plan, a, n, bcast, st, [&](int g, int cnt) {
    return fa_tgpu16::launch(a, g, cnt, plan->elem, plan->out_elem == FA_ELEM_F32, st);
  });
}

// the 16-bit kernels (fedagg_h16.hip) over the plan's one table, then the
// broadcast's flat copy of the result bucket
hipError_t run_h16(const fa_plan* plan, ReduceArgs& a, int n, bool weighted, bool bcast,
                   hipStream_t st) {
  a.nscalar = plan->ns;
  a.sidx = plan->d_sidx;
  a.ntiles = plan->nt;
  hipError_t e = fa_h16::launch(a, plan->nt, plan->elem, plan->vec_u, weighted,
                                plan->out_elem == FA_ELEM_F32, st);
  if (e == hipSuccess && bcast) e = launch_bcast(plan, a, n, plan->nt, st);
  return e;
}

// the table and kernel form the launch rules choose (fa_host::select_launch);
// the broadcast is its own launch after the reduce
hipError_t run_default(const fa_plan* plan, ReduceArgs& a, int n, bool weighted, bool bcast,
                       hipStream_t st) {
  const fa_host::Launch L = fa_host::select_launch(*plan, n, weighted, kernel_slots);
  a.tiles = L.table >= 0 ? plan->d_bal[L.table] : L.alt ? plan->d_tiles_alt : plan->d_tiles;
  a.sidx = L.alt && plan->d_sidx ? plan->d_sidx + plan->sidx_alt_off : plan->d_sidx;
  a.nscalar = L.ns;
  a.ntiles = L.nt;
  hipError_t e = launch_reduce(a, L.nt, L.vec_u, st, L.batch, L.pipe);
  if (e == hipSuccess && bcast) e = launch_bcast(plan, a, n, L.nt, st);
  return e;
}
}  // namespace

int fa_reduce_tab(const fa_plan* plan, const float* const* c32, const int64_t* const* c64, int n,
                  const float* weights, void* ctable, float* out32, int64_t* out64,
                  unsigned flags, void* stream) {
  if (!plan) return set_err(FA_E_INVAL, "fa_reduce: plan is NULL");
  if (n < 1) return set_err(FA_E_INVAL, "fa_reduce: need at least one client (n=%d)", n);
  if (n > FA_MAX_CLIENTS)
    return set_err(FA_E_RANGE, "fa_reduce: n=%d exceeds FA_MAX_CLIENTS=%d", n, FA_MAX_CLIENTS);
  if (flags & ~(FA_F_BCAST | FA_F_SUM_ONLY | FA_F_BCAST_ONLY))
    return set_err(FA_E_INVAL, "fa_reduce: bad flags");
  const bool tgpu = plan->tgpu();
  if (tgpu && weights)
    return set_err(FA_E_INVAL, "fa_reduce: the torch-GPU order is the reference's unweighted mean");
  const bool h16 = plan->elem != FA_ELEM_F32;
  if (h16 && (flags & FA_F_SUM_ONLY))
    return set_err(FA_E_INVAL, "fa_reduce: FA_F_SUM_ONLY is not defined for a 16-bit plan (the "
                               "ordered fp32 sum has no 16-bit slot to go to)");
  if (h16 && (flags & (FA_F_BCAST | FA_F_BCAST_ONLY)) && !plan->flat_bcast)
    return set_err(FA_E_INVAL, "fa_reduce: a 16-bit plan broadcasts the bucket's bytes flat (a "
                               "mixed plan: narrows the whole fp32 bucket) and needs "
                               "FA_PLAN_GAPS_ARE_PADDING with full coverage");
  if (n > kInline && ctable && ((uintptr_t)ctable & 7))
    return set_err(FA_E_ALIGN, "fa_reduce_tab: table not 8-B aligned");
  if (plan->info.ntiles == 0) return FA_OK;
  ReduceArgs a;
  memset(&a, 0, sizeof a);
  a.tiles = plan->d_tiles;
  a.out32 = out32;
  a.out64 = out64;
  a.n = n;
  a.n_total = n;
  // every reduce's broadcast is a launch of its own: FA_F_BCAST reaches the
  // kernels through launch_bcast only
  a.flags = (flags & ~FA_F_BCAST) | (weights ? 0x100u : 0u);
  const bool need32 = plan->has32, need64 = plan->has64;
  if (need32) {
    if (!c32 || !out32) return set_err(FA_E_INVAL, "fa_reduce: fp32 buckets required");
    if (!aligned16(out32)) return set_err(FA_E_ALIGN, "fa_reduce: out32 not 16-B aligned");
    for (int i = 0; i < n; ++i) {
      if (!c32[i]) return set_err(FA_E_INVAL, "fa_reduce: client %d fp32 bucket NULL", i);
      if (!aligned16(c32[i]))
        return set_err(FA_E_ALIGN, "fa_reduce: client %d fp32 bucket not 16-B aligned", i);
    }
  }
  if (need64) {
    if (!c64 || !out64) return set_err(FA_E_INVAL, "fa_reduce: int64 buckets required");
    for (int i = 0; i < n; ++i)
      if (!c64[i]) return set_err(FA_E_INVAL, "fa_reduce: client %d int64 bucket NULL", i);
  }
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != plan->device)
    return set_err(FA_E_INVAL, "fa_reduce: plan built on device %d, current device %d",
                   plan->device, dev);
  const bool bcast_only = (flags & FA_F_BCAST_ONLY) != 0, bcast = (flags & FA_F_BCAST) != 0;
  // refused before the table is filled: no refusal launches or allocates
  if (tgpu && !bcast_only && n != plan->order_n)
    return set_err(FA_E_INVAL, "fa_reduce: torch-GPU-order plan cut for n=%d, called with n=%d",
                   plan->order_n, n);
  hipStream_t st = (hipStream_t)stream;
  ClientTable tab{st};
  hipError_t e = tab.fill(a, need32 ? c32 : nullptr, need64 ? c64 : nullptr, n, weights, ctable);
  if (e != hipSuccess)
    return set_err(FA_E_HIP, "fa_reduce: client pointer table: %s", hipGetErrorString(e));
  static const char* const kWhat[] = {"reduce launch", "16-bit reduce launch",
                                      "torch-GPU-order launch", "16-bit torch-GPU-order launch"};
  const char* what = bcast_only ? "broadcast launch" : kWhat[(int)plan->family];
  const bool w = weights != nullptr;
  if (bcast_only) {
    e = run_bcast_only(plan, a, n, st);
  } else {
    switch (plan->family) {
      case FaFamily::kDefault: e = run_default(plan, a, n, w, bcast, st); break;
      case FaFamily::kH16: e = run_h16(plan, a, n, w, bcast, st); break;
      case FaFamily::kTgpu: e = run_tgpu(plan, a, n, bcast, st); break;
      case FaFamily::kTgpu16: e = run_tgpu16(plan, a, n, bcast, st); break;
    }
  }
  e = tab.done(e);
  if (e != hipSuccess) return set_err(FA_E_HIP, "%s: %s", what, hipGetErrorString(e));
  return FA_OK;
}

namespace {
// fa_reduce_chain (`who` names it; fp32 plans) and fa_reduce_chain_elem's
// 16-bit path (`h16`: an h16-family plan, the kernels of fedagg_chain16.hip):
// one set of checks in one order, every refusal before anything is launched.
int reduce_chain(const char* who, bool h16, const fa_plan* plan, const void* const* c, int n,
                 const float* weights, const fa_chain* ch, void* out, unsigned flags,
                 void* stream) {
  if (!plan || !ch) return set_err(FA_E_INVAL, "%s: plan/chain is NULL", who);
  if (flags & ~FA_F_SUM_ONLY) return set_err(FA_E_INVAL, "%s: bad flags", who);
  const int nt = ch->n_total;
  if (nt < 1 || nt > FA_MAX_CLIENTS)
    return set_err(FA_E_RANGE, "%s: n_total=%d outside 1..%d", who, nt, FA_MAX_CLIENTS);
  if (n < 1 || ch->row0 < 0 || ch->row0 + n > nt)
    return set_err(FA_E_INVAL, "%s: rows [%d,+%d) outside the %d-row reduction", who, ch->row0, n,
                   nt);
  if (!h16 && plan->elem != FA_ELEM_F32)
    return set_err(FA_E_INVAL, "%s: not defined for a 16-bit plan (the state planes "
                               "are fp32; chain fp32 buckets)", who);
  if (h16 && plan->family != FaFamily::kH16)
    return set_err(FA_E_INVAL, "%s: not defined for a torch-GPU-order plan (the chain carries "
                               "the cascade of torch's CPU order)", who);
  if (h16 && (flags & FA_F_SUM_ONLY) && plan->out_elem != FA_ELEM_F32)
    return set_err(FA_E_INVAL, "%s: FA_F_SUM_ONLY is not defined for a 16-bit result (the "
                               "ordered fp32 sum has no 16-bit slot to go to)", who);
  if (plan->has64 || plan->info.ntiles_tail > 0)
    return set_err(FA_E_INVAL,
                   "%s: the plan holds scalar tiles (tails, M==1, int64); chain "
                   "plans carry vector tiles only (scalar columns travel raw, fedagg_comm.h)",
                   who);
  const unsigned lin = fa_chain_levels(ch->row0, nt);
  const unsigned lout = fa_chain_levels(ch->row0 + n, nt);
  if (lin && !ch->state_in)
    return set_err(FA_E_INVAL, "%s: rows 0..%d-1 leave a state: state_in required", who, ch->row0);
  if (!ch->state_out && !out) return set_err(FA_E_INVAL, "%s: need state_out or out32", who);
  if (ch->state_out && ch->row0 + n == nt)
    return set_err(FA_E_INVAL, "%s: the last segment finishes (state_out NULL)", who);
  if (!ch->state_out && ch->row0 + n != nt)
    return set_err(FA_E_INVAL, "%s: only the last segment (rows ..%d) finishes", who, nt - 1);
  const bool st = ch->state_in || ch->state_out;
  if (st && (ch->plane < plan->info.f32_numel || ch->plane % 4))
    return set_err(FA_E_INVAL, "%s: plane=%lld must be >= %lld and a multiple of 4", who,
                   (long long)ch->plane, (long long)plan->info.f32_numel);
  if ((ch->state_in && !aligned16(ch->state_in)) || (ch->state_out && !aligned16(ch->state_out)) ||
      (out && !aligned16(out)))
    return set_err(FA_E_ALIGN, "%s: state/out buffers not 16-B aligned", who);
  if (plan->info.ntiles == 0) return FA_OK;
  if (!c) return set_err(FA_E_INVAL, "%s: %s buckets required", who, h16 ? "16-bit" : "fp32");
  for (int i = 0; i < n; ++i)
    if (!c[i] || !aligned16(c[i]))
      return set_err(FA_E_ALIGN, "%s: client %d bucket NULL or not 16-B aligned", who, i);
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != plan->device)
    return set_err(FA_E_INVAL, "%s: plan built on device %d, current device %d", who,
                   plan->device, dev);
  ReduceArgs a;
  memset(&a, 0, sizeof a);
  a.tiles = plan->d_tiles;
  a.out32 = (float*)out;  // (a 16-bit plan: the 16-bit result bucket)
  a.n = n;
  a.n_total = nt;
  a.row0 = ch->row0;
  a.st_in = lin ? ch->state_in : nullptr;
  a.st_out = ch->state_out;
  a.lev_in = (int)lin;
  a.lev_out = (int)lout;
  a.plane = ch->plane;
  a.flags = flags | (weights ? 0x100u : 0u);
  a.ntiles = plan->nt;
  hipStream_t s = (hipStream_t)stream;
  ClientTable tab{s};
  hipError_t e = tab.fill(a, (const float* const*)c, nullptr, n, weights, nullptr);
  if (e != hipSuccess)
    return set_err(FA_E_HIP, "%s: client pointer table: %s", who, hipGetErrorString(e));
  e = tab.done(h16 ? fa_chain16::launch(a, a.ntiles, plan->elem, plan->vec_u, weights != nullptr,
                                        plan->out_elem == FA_ELEM_F32, s)
                   : launch_chain(a, a.ntiles, plan->vec_u, s));
  if (e != hipSuccess)
    return set_err(FA_E_HIP, "%s: %s", h16 ? "16-bit chain launch" : "chain launch",
                   hipGetErrorString(e));
  return FA_OK;
}
}  // namespace

int fa_reduce_chain(const fa_plan* plan, const float* const* c32, int n, const float* weights,
                    const fa_chain* ch, float* out32, unsigned flags, void* stream) {
  return reduce_chain("fa_reduce_chain", false, plan, (const void* const*)c32, n, weights, ch,
                      out32, flags, stream);
}

int fa_reduce_chain_elem(const fa_plan* plan, const void* const* c, int n, const float* weights,
                         const fa_chain* ch, void* out, unsigned flags, void* stream) {
  // an fp32 plan (and a NULL one's refusal): fa_reduce_chain exactly
  if (!plan || plan->elem == FA_ELEM_F32)
    return fa_reduce_chain(plan, (const float* const*)c, n, weights, ch, (float*)out, flags,
                           stream);
  return reduce_chain("fa_reduce_chain_elem", true, plan, c, n, weights, ch, out, flags, stream);
}

int fa_mean_f32(const float* const* clients, int n, int64_t numel, float* out,
                const fa_seg* segs, int nseg, void* stream) {
  fa_plan* p = nullptr;
  int rc = cached_plan(segs, nseg, numel, nullptr, 0, 0, &p);
  if (rc) return rc;
  return fa_reduce(p, clients, nullptr, n, nullptr, out, nullptr, 0, stream);
}

int fa_weighted_f32(const float* const* clients, const float* w, int n, int64_t numel,
                    float* out, const fa_seg* segs, int nseg, void* stream) {
  if (!w) return set_err(FA_E_INVAL, "fa_weighted_f32: weights NULL");
  fa_plan* p = nullptr;
  int rc = cached_plan(segs, nseg, numel, nullptr, 0, 0, &p);
  if (rc) return rc;
  return fa_reduce(p, clients, nullptr, n, w, out, nullptr, 0, stream);
}

int fa_mean_i64_trunc(const int64_t* const* clients, int n, int64_t numel, int64_t* out,
                      const fa_seg* segs, int nseg, void* stream) {
  fa_plan* p = nullptr;
  int rc = cached_plan(nullptr, 0, 0, segs, nseg, numel, &p);
  if (rc) return rc;
  return fa_reduce(p, nullptr, clients, n, nullptr, nullptr, out, 0, stream);
}

int fa_div_f32(const float* x, float d, float* out, int64_t numel, void* stream) {
  if (numel < 0 || (numel > 0 && (!x || !out))) return set_err(FA_E_INVAL, "fa_div_f32: bad args");
  if (numel == 0) return FA_OK;
  hipLaunchKernelGGL(div_f32_kernel, dim3(grid_for(numel, kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, x, d, out, numel);
  HIP_TRY(hipGetLastError());
  return FA_OK;
}

int fa_div_trunc_i64(const float* x, float d, int64_t* out, int64_t numel, void* stream) {
  if (numel < 0 || (numel > 0 && (!x || !out)))
    return set_err(FA_E_INVAL, "fa_div_trunc_i64: bad args");
  if (numel == 0) return FA_OK;
  hipLaunchKernelGGL(div_trunc_i64_kernel, dim3(grid_for(numel, kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, x, d, out, numel);
  HIP_TRY(hipGetLastError());
  return FA_OK;
}

int fa_broadcast_f32(const float* src, float* const* dst, int n, int64_t numel, void* stream) {
  if (n < 0 || n > FA_MAX_CLIENTS) return set_err(FA_E_RANGE, "fa_broadcast_f32: n=%d", n);
  if (numel < 0 || (numel > 0 && (!src || (n > 0 && !dst))))
    return set_err(FA_E_INVAL, "fa_broadcast_f32: bad args");
  if (n == 0 || numel == 0) return FA_OK;
  if (!aligned16(src)) return set_err(FA_E_ALIGN, "fa_broadcast_f32: src not 16-B aligned");
  for (int i = 0; i < n; ++i)
    if (!dst[i] || !aligned16(dst[i]))
      return set_err(FA_E_ALIGN, "fa_broadcast_f32: dst %d NULL or unaligned", i);
  for (int i0 = 0; i0 < n; i0 += kBcastInline) {
    BcastArgs a;
    memset(&a, 0, sizeof a);
    a.src = src;
    a.n = std::min(kBcastInline, n - i0);
    for (int i = 0; i < a.n; ++i) a.dst[i] = dst[i0 + i];
    const int64_t parts = std::max<int64_t>(1, (numel / 4 + 2 * kBlock - 1) / (2 * kBlock));
    const uint32_t groups = (uint32_t)((a.n + kBcastGroupMax - 1) / kBcastGroupMax);
    const uint32_t gsize = (uint32_t)((a.n + groups - 1) / groups);
    if (parts * groups > (int64_t)UINT32_MAX)
      return set_err(FA_E_RANGE, "fa_broadcast_f32: numel=%lld", (long long)numel);
    const unsigned grid = (unsigned)std::min<int64_t>(parts * groups, 1ll << 30);
    hipLaunchKernelGGL(bcast_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a, numel,
                       (uint32_t)parts, groups, gsize);
    HIP_TRY(hipGetLastError());
  }
  return FA_OK;
}

int fa_write_probe_f32(float* const* dst, int n, int64_t numel, unsigned seed, void* stream) {
  if (n < 0 || n > kBcastInline) return set_err(FA_E_RANGE, "fa_write_probe_f32: n=%d", n);
  if (numel < 0 || (numel > 0 && n > 0 && !dst))
    return set_err(FA_E_INVAL, "fa_write_probe_f32: bad args");
  if (n == 0 || numel < 4) return FA_OK;
  BcastArgs a;
  memset(&a, 0, sizeof a);
  a.n = n;
  for (int i = 0; i < n; ++i) {
    if (!dst[i] || !aligned16(dst[i]))
      return set_err(FA_E_ALIGN, "fa_write_probe_f32: dst %d NULL or unaligned", i);
    a.dst[i] = dst[i];
  }
  const int64_t parts = (numel / 4 + kBlock - 1) / kBlock;
  const uint32_t groups = (uint32_t)((n + kBcastGroupMax - 1) / kBcastGroupMax);
  const uint32_t gsize = (uint32_t)((n + groups - 1) / groups);
  if (parts * groups > (int64_t)UINT32_MAX)
    return set_err(FA_E_RANGE, "fa_write_probe_f32: numel=%lld", (long long)numel);
  hipLaunchKernelGGL(write_probe_kernel, dim3((unsigned)(parts * groups)), dim3(kBlock), 0,
                     (hipStream_t)stream, a, numel, (uint32_t)parts, groups, gsize, seed);
  HIP_TRY(hipGetLastError());
  return FA_OK;
}

int fa_synth_fill_f32(float* dst, int64_t numel, int key_index, int client, float mu,
                      float sigma, int mode, void* stream) {
  if (numel < 0 || (numel > 0 && !dst)) return set_err(FA_E_INVAL, "fa_synth_fill_f32: bad args");
  if (numel == 0) return FA_OK;
  // the generator's third constant, rounded exactly as synth.key_consts does
  volatile float s = sigma, c = 0.01f;
  const float dsig = s * c;
  hipLaunchKernelGGL(synth_f32_kernel, dim3(grid_for(numel, kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, dst, numel, key_index, client, mu, sigma, dsig, mode);
  HIP_TRY(hipGetLastError());
  return FA_OK;
}

int fa_synth_fill_i64(int64_t* dst, int64_t numel, int key_index, int client, int mode,
                      void* stream) {
  if (numel < 0 || (numel > 0 && !dst)) return set_err(FA_E_INVAL, "fa_synth_fill_i64: bad args");
  if (numel == 0) return FA_OK;
  hipLaunchKernelGGL(synth_i64_kernel, dim3(grid_for(numel, kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, dst, numel, key_index, client, mode);
  HIP_TRY(hipGetLastError());
  return FA_OK;
}

int fa_read_probe_f32(const float* src, int64_t numel, float* out, int grid, void* stream) {
  if (numel < 4 || !src || !out || grid < 0) return set_err(FA_E_INVAL, "fa_read_probe_f32: bad args");
  if (!aligned16(src)) return set_err(FA_E_ALIGN, "fa_read_probe_f32: unaligned");
  if (grid == 0) {  // one 2048-float tile per workgroup (whole float4s only)
    const int64_t nv = numel / 4, g = (nv + 2 * kBlock - 1) / (2 * kBlock);
    if (g > 0x7fffffff) return set_err(FA_E_RANGE, "fa_read_probe_f32: %lld floats", (long long)numel);
    hipLaunchKernelGGL(read_tile_kernel, dim3((unsigned)g), dim3(kBlock), 0, (hipStream_t)stream,
                       src, nv, out);
  } else {
    hipLaunchKernelGGL(read_probe_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, src,
                       numel / 4, out);
  }
  HIP_TRY(hipGetLastError());
  return FA_OK;
}

int fa_narrow_f32(const float* src, void* dst, int elem, int64_t numel, void* stream) {
  if (elem != FA_ELEM_F16 && elem != FA_ELEM_BF16)
    return set_err(FA_E_INVAL, "fa_narrow_f32: elem must be FA_ELEM_F16 or FA_ELEM_BF16 (got %d)",
                   elem);
  if (numel < 0) return set_err(FA_E_INVAL, "fa_narrow_f32: numel=%lld", (long long)numel);
  if (numel == 0) return FA_OK;
  if (!src || !dst) return set_err(FA_E_INVAL, "fa_narrow_f32: NULL pointer");
  if (!aligned16(src) || !aligned16(dst))
    return set_err(FA_E_INVAL, "fa_narrow_f32: src / dst not 16-B aligned");
  const hipError_t e = fa_h16::narrow_range(src, dst, elem, numel, (hipStream_t)stream);
  if (e != hipSuccess) return set_err(FA_E_HIP, "fa_narrow_f32: %s", hipGetErrorString(e));
  return FA_OK;
}

int fa_copy_f32(const float* src, float* dst, int64_t numel, void* stream) {
  if (numel < 0 || (numel > 0 && (!src || !dst))) return set_err(FA_E_INVAL, "fa_copy_f32: bad args");
  if (numel == 0) return FA_OK;
  if (!aligned16(src) || !aligned16(dst)) return set_err(FA_E_ALIGN, "fa_copy_f32: unaligned");
  const int64_t grid = std::max<int64_t>(1, (numel / 4 + kBlock - 1) / kBlock);
  if (grid > 0x7fffffff) return set_err(FA_E_RANGE, "fa_copy_f32: %lld floats", (long long)numel);
  hipLaunchKernelGGL(copy_kernel, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, src,
                     dst, numel);
  HIP_TRY(hipGetLastError());
  return FA_OK;
}

}  // extern "C"
