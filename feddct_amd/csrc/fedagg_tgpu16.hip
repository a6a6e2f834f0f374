// fedagg_tgpu16.hip — torch-ROCm's GPU summation order over fp16 / bf16
// buckets (fa_plan_create_order_elem).  The reference's line on device
// tensors of model.half() / model.bfloat16() clients,
//
//     torch.stack([m.state_dict()[k].float() for m in clients], 0).mean(0)
//
// followed by load_state_dict's copy_ into the 16-bit key: every value is
// widened exactly to fp32, the stacked tensor is fp32, so torch's reduction
// is the fp32 one of fedagg.hip's "torch-ROCm's GPU order" (row r into part
// r % S, accumulator (r / S) % 4, ((a0 + a1) + a2) + a3, the halving tree
// over the parts; the lane tree for M == 1), the sum is multiplied by
// float(M) / float(N M), and the fp32 value is rounded to nearest-even into
// the key's type.  The kernels read the clients' 16-bit buckets directly and
// write a 16-bit result.  WIDE instances (fa_plan_create_order_elem_out, an
// fp32 master global over 16-bit clients) differ in the finish alone: the
// fp32 value sum times factor is stored unrounded into an fp32 bucket at the
// same element offsets, and fedagg_h16.hip's narrowing broadcast then rounds
// it into the clients' buckets.
//
// Its own translation unit and its own kernel family (DESIGN §4.1:
// tgpu_kernel and reduce_impl.h are not templated on the element type).  The
// order functions tgpu_outer / tgpu_inner / tgpu_inner_vec are restated here
// word for word from fedagg.hip, which stays textually alone.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "conv16.h"
#include "tgpu16.h"

namespace fa_tgpu16 {
using namespace fa_k;
using fa_h16::kTile;
using fa_h16::kVec;
using fa_h16::narrow;
using fa_h16::narrow8;
using fa_h16::u4;
using fa_h16::widen;
using fa_h16::widen8;

typedef __attribute__((address_space(1))) const u4 gcu4;

// 16-B non-temporal load of vector `vidx` (8 elements) past a uniform base.
__device__ __forceinline__ u4 ldu4(const uint16_t* base, uint32_t vidx) {
  return __builtin_nontemporal_load((gcu4*)base + vidx);
}
// The result store: a buffer store with the sc1 policy bit (reduce_impl.h
// st_out, fedagg_h16.hip st_sc1: the broadcast reads the result next).
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
// Client i's 16-bit bucket through scalar loads only (reduce_impl.h sptr32).
__device__ __forceinline__ const uint16_t* sptr16(KArgs& a, int i) {
  return (const uint16_t*)sptr32(a, i);
}

// The fp32 result, sum times factor, pinned in a register before it is
// narrowed: with fp16 the compiler otherwise folds the multiply and the
// conversion into one mixed-precision multiply-add that rounds once, from the
// exact product, where torch rounds the fp32 mean (prox_h16.hip pin).
__device__ __forceinline__ float mean32(float s, float fac) {
  float x = __fmul_rn(s, fac);
  asm volatile("" : "+v"(x));
  return x;
}
__device__ __forceinline__ f4 mean32x4(f4 s, float fac) {
  return f4{mean32(s.x, fac), mean32(s.y, fac), mean32(s.z, fac), mean32(s.w, fac)};
}
// ... of a WIDE instance: stored as it is, so there is nothing to fold into
__device__ __forceinline__ f4 wide32x4(f4 s, float fac) {
  return f4{__fmul_rn(s.x, fac), __fmul_rn(s.y, fac), __fmul_rn(s.z, fac), __fmul_rn(s.w, fac)};
}

// The value the scalar orders read from a 16-bit bucket: widened exactly.
template <int EL>
struct Src16 {
  KArgs& a;
  __device__ float operator()(int i, int64_t e) const {
    return widen<EL>(((const uint16_t*)cptr32(a, i))[e]);
  }
};

// ------------------------------------------ the order (fedagg.hip's words) --
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

// M == 1 with N >= 128: the input-vectorised form (fedagg.hip tgpu_inner_vec)
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

// ------------------------------------------------------------ wide tiles ---
// A lane's 8 adjacent columns as two f4 halves.
struct F8 {
  f4 lo, hi;
};
__device__ __forceinline__ F8 zero8() {
  const f4 z = {0.f, 0.f, 0.f, 0.f};
  return F8{z, z};
}
__device__ __forceinline__ F8 add8(F8 x, F8 y) { return F8{add4(x.lo, y.lo), add4(x.hi, y.hi)}; }
// factor, round to nearest-even, one 16-B store (WIDE: the lane's 8 fp32
// values as two 16-B stores at float offset start + 8 vi — the form
// finish8_xchg below replaces on wide tiles)
template <int EL, bool WIDE>
__device__ __forceinline__ void finish8(KArgs& a, int64_t start, uint32_t vi, F8 r, float fac) {
  if constexpr (WIDE) {
    st_sc1_f4(a.out32 + start, 32 * vi, wide32x4(r.lo, fac));
    st_sc1_f4(a.out32 + start, 32 * vi + 16, wide32x4(r.hi, fac));
  } else {
    st_sc1((uint16_t*)a.out32 + start, vi, narrow8<EL>(mean32x4(r.lo, fac), mean32x4(r.hi, fac)));
  }
}

// The WIDE finish after an exchange inside the wave (fedagg_h16.hip
// tile_vec16's): a lane's 8 fp32 results are 32 B, and stored from the lane
// that summed them each store instruction covers only every other 16 B of the
// wave's 2 KB.  For store s, lane t takes half t & 1 of lane 32 s + t / 2, and
// each store instruction writes 1 KB contiguous, as the 16-bit result store
// does.  Every lane of the workgroup takes part (one past the tile's end holds
// +0 sums); a store goes out when its SOURCE lane is inside.  Stored from
// the summing lane the launch ran 13.2 us behind at N = 5 (39.5 against
// 26.3 us), 9.5 us at N = 20, 6.6 us at N = 32 and 3 us at N = 64
// (profiles/tgpu16_master_finish.jsonl).
// (FA_TGPU16_WIDE_XCHG: 0 stores from the summing lane, for that A/B:
// tools/tgpu16_ab.py kernel --master 1 --tree)
#ifndef FA_TGPU16_WIDE_XCHG
#define FA_TGPU16_WIDE_XCHG 1
#endif
__device__ __forceinline__ f4 shfl4(f4 v, int src) {
  return f4{__shfl(v.x, src, 64), __shfl(v.y, src, 64), __shfl(v.z, src, 64),
            __shfl(v.w, src, 64)};
}
template <bool FULL>
__device__ __forceinline__ void finish8_xchg(KArgs& a, int64_t start, int count, F8 r, float fac) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wv0 = threadIdx.x - lane;  // the wave's first vector
  const f4 lo = wide32x4(r.lo, fac), hi = wide32x4(r.hi, fac);
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const uint32_t src = 32 * s + (lane >> 1);
    const f4 l = shfl4(lo, (int)src), h = shfl4(hi, (int)src);
    const f4 v = (lane & 1) ? h : l;
    if (FULL || (int)(kVec * (wv0 + src)) < count)
      st_sc1_f4(a.out32 + start, 32 * wv0 + 1024 * s + 16 * lane, v);
  }
}

// S = 1 or 2 over tiles of up to 2048 elements, one 16-B load per lane per
// row, with the client loop (fedagg.hip tgpu_wide_loop's accumulator
// assignment): rows in slot order, row b + 1's load issued before row b's
// adds, row r into part r % S and that part's accumulator (r / S) % 4; 4 S
// rows per pass keep the accumulator index static.  A lane past a partial
// tile's end loads nothing and stores nothing.
// PASSES = false, the S = 1 group's launch: one loop over the rows, each step
// under its own end test, the row in flight handed on as cur = nxt (56 VGPRs,
// eight workgroups per CU).
// PASSES = true, the S = 2 group's launch: whole passes of R rows run without
// a per-row end test, the two rows in flight in two registers with static
// roles; the compiler then issues a pass's R loads together.  In the first
// form this launch's kernel (130 VGPRs with its riders' paths, three or four
// workgroups per CU) waited for row b + 1 in the middle of row b's adds — the
// copy cur = nxt of a load still in flight — so nothing overlapped: 145.8 us
// at N = 32 against 113.0 us in this form; the S = 1 launch is the other way
// round, 71.5 against 79.6 us at N = 20.
// (FA_TGPU16_S1_PASSES / FA_TGPU16_S2_PASSES: the form of each launch, for
// that A/B: tools/tgpu16_ab.py kernel --tree)
#ifndef FA_TGPU16_S1_PASSES
#define FA_TGPU16_S1_PASSES 0
#endif
#ifndef FA_TGPU16_S2_PASSES
#define FA_TGPU16_S2_PASSES 1
#endif
template <int EL, int S, bool FULL, bool PASSES, bool WIDE>
__device__ __forceinline__ void wide16(KArgs& a, int64_t start, int count, float fac) {
  static_assert(S == 1 || S == 2, "row split of the wide loop");
  constexpr int R = 4 * S;
  const uint32_t vi = threadIdx.x;
  const bool ok = FULL || (int)(kVec * vi) < count;
  const u4 zero = u4{0u, 0u, 0u, 0u};
  F8 acc[R];
#pragma unroll
  for (int k = 0; k < R; ++k) acc[k] = zero8();
  const int n = a.n;
  if constexpr (!PASSES) {
    u4 cur = (FULL || ok) ? ldu4(sptr16(a, 0) + start, vi) : zero, nxt = zero;
    for (int b0 = 0; b0 < n; b0 += R) {
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int b = b0 + k;
        if (b < n) {
          if (b + 1 < n) nxt = (FULL || ok) ? ldu4(sptr16(a, b + 1) + start, vi) : zero;
          F8 x;
          widen8<EL>(cur, &x.lo, &x.hi);
          const int ai = (k % S) * 4 + ((k / S) & 3);
          acc[ai] = add8(acc[ai], x);
          cur = nxt;
        }
      }
    }
  } else {
    u4 ring[2] = {zero, zero};  // row b in ring[b % 2] (R is even)
    if (FULL || ok) ring[0] = ldu4(sptr16(a, 0) + start, vi);
    int b0 = 0;
    for (; b0 + R <= n; b0 += R) {
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int b = b0 + k;
        if ((k + 1 < R || b + 1 < n) && (FULL || ok))
          ring[(k + 1) % 2] = ldu4(sptr16(a, b + 1) + start, vi);
        F8 x;
        widen8<EL>(ring[k % 2], &x.lo, &x.hi);
        const int ai = (k % S) * 4 + ((k / S) & 3);
        acc[ai] = add8(acc[ai], x);
      }
    }
    if (b0 < n) {  // the last, partial pass: at most R - 1 rows
#pragma unroll
      for (int k = 0; k < R - 1; ++k) {
        const int b = b0 + k;
        if (b < n) {
          if (b + 1 < n && (FULL || ok)) ring[(k + 1) % 2] = ldu4(sptr16(a, b + 1) + start, vi);
          F8 x;
          widen8<EL>(ring[k % 2], &x.lo, &x.hi);
          const int ai = (k % S) * 4 + ((k / S) & 3);
          acc[ai] = add8(acc[ai], x);
        }
      }
    }
  }
  if constexpr (WIDE && FA_TGPU16_WIDE_XCHG != 0) {
    F8 r = add8(add8(add8(acc[0], acc[1]), acc[2]), acc[3]);
    if constexpr (S == 2) r = add8(r, add8(add8(add8(acc[4], acc[5]), acc[6]), acc[7]));
    finish8_xchg<FULL>(a, start, count, r, fac);
    return;
  }
  if (!FULL && !ok) return;
  F8 r = add8(add8(add8(acc[0], acc[1]), acc[2]), acc[3]);
  if constexpr (S == 2) r = add8(r, add8(add8(add8(acc[4], acc[5]), acc[6]), acc[7]));
  finish8<EL, WIDE>(a, start, vi, r, fac);
}

// ---------------------------------------------------------- S >= 4 tiles ---
// fedagg.hip tgpu_outer4's shape: 4 columns per lane (one 8-B load per row),
// a tile of up to 2048 elements in two passes of the workgroup.  With 8
// columns per lane the S parts' values alone are 8 S registers: the S = 8
// instance held 256 VGPRs and the S = 16 one spilled (the compiler's resource
// report), so these tiles take 4.  Part y's p-th row is y + p S, row p into
// accumulator p % 4; B rows' loads issued, then added in row order; the parts
// meet in the halving tree.
typedef uint32_t u2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) const u2 gcu2;
template <int EL>
__device__ __forceinline__ f4 widen4(u2 w) {
  float f[4];
  fa_h16::widen2<EL>(w.x, &f[0], &f[1]);
  fa_h16::widen2<EL>(w.y, &f[2], &f[3]);
  return f4{f[0], f[1], f[2], f[3]};
}
template <int EL, int S>
__device__ __forceinline__ f4 outer4(KArgs& a, int64_t start, uint32_t v, int n) {
  f4 val[S];
#pragma unroll
  for (int y = 0; y < S; ++y) {
    const f4 z = {0.f, 0.f, 0.f, 0.f};
    f4 acc[4] = {z, z, z, z};
    const int np = (n - y + S - 1) / S;
    constexpr int B = S >= 8 ? 4 : 8;  // rows in flight (register budget of val[S])
    int p = 0;
    for (; p + B <= np; p += B) {
      u2 x[B];
#pragma unroll
      for (int i = 0; i < B; ++i)
        x[i] = __builtin_nontemporal_load((gcu2*)(sptr16(a, y + (p + i) * S) + start) + v);
#pragma unroll
      for (int i = 0; i < B; ++i) acc[i & 3] = add4(acc[i & 3], widen4<EL>(x[i]));
    }
    if (p < np) {  // p % 4 == 0 here: row p + i goes into accumulator i & 3
      u2 x[B];
#pragma unroll
      for (int i = 0; i < B; ++i)
        if (p + i < np)
          x[i] = __builtin_nontemporal_load((gcu2*)(sptr16(a, y + (p + i) * S) + start) + v);
#pragma unroll
      for (int i = 0; i < B; ++i)
        if (p + i < np) acc[i & 3] = add4(acc[i & 3], widen4<EL>(x[i]));
    }
    val[y] = add4(add4(add4(acc[0], acc[1]), acc[2]), acc[3]);
  }
#pragma unroll
  for (int off = S / 2; off > 0; off /= 2)
#pragma unroll
    for (int y = 0; y < off; ++y) val[y] = add4(val[y], val[y + off]);
  return val[0];
}

// A V tile (4 elements per lane per pass, 8-B sc1 result stores; WIDE: one
// 16-B store of the 4 fp32 values) and a scalar tile (one element per lane;
// WIDE: a 4-B store) of row split S.
template <int EL, int S, bool WIDE>
__device__ __forceinline__ void v_tile(KArgs& a, const Tile& t, float fac) {
  if constexpr (WIDE) {
    for (int h = 0; h < kTile / (4 * kBlock); ++h) {
      const uint32_t v = threadIdx.x + h * kBlock;
      if ((int)(v * 4) >= t.count) return;
      st_sc1_f4(a.out32 + t.start, 16 * v, wide32x4(outer4<EL, S>(a, t.start, v, a.n), fac));
    }
    return;
  }
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      (uint16_t*)a.out32 + t.start, (short)0, 0x7fffffff, 0x00020000);
  for (int h = 0; h < kTile / (4 * kBlock); ++h) {
    const uint32_t v = threadIdx.x + h * kBlock;
    if ((int)(v * 4) >= t.count) return;
    const f4 r = mean32x4(outer4<EL, S>(a, t.start, v, a.n), fac);
    const u2 w = u2{fa_h16::narrow2<EL>(r.x, r.y), fa_h16::narrow2<EL>(r.z, r.w)};
    __builtin_amdgcn_raw_buffer_store_b64(w, rs, (int)(8 * v), 0, 16);
  }
}
template <int EL, int S, bool WIDE>
__device__ __forceinline__ void scalar_tile(KArgs& a, const Tile& t, float fac) {
  const int j = threadIdx.x;
  if (j >= t.count) return;
  const int64_t e = t.start + j;
  if ((t.kind & 0xFF) == K_F32_TGPU) {
    const float s = tgpu_outer<Src16<EL>, S>(Src16<EL>{a}, e, a.n);
    if constexpr (WIDE) a.out32[e] = __fmul_rn(s, fac);
    else ((uint16_t*)a.out32)[e] = (uint16_t)narrow<EL>(mean32(s, fac));
  } else {
    a.out64[e] = (int64_t)__fmul_rn(tgpu_outer<SrcI64, S>(SrcI64{a}, e, a.n), fac);
  }
}

// One instantiation per element type and row split S = 1 << LS, as
// fedagg.hip's tgpu_kernel<LS>: the plan groups its tiles by S and launches
// each group; inner tiles (M == 1) ride in the LS = 0 group; when the S = 2
// group is the largest, the S = 1 and S = 4 tiles and the inner tiles ride
// in its launch.  WIDE: the fp32-store form of the same kernel.
template <int EL, int LS, bool WIDE>
__global__ __launch_bounds__(kBlock) void tgpu16_kernel(ReduceArgs args) {
  (void)args;
  constexpr int S = 1 << LS;
  KArgs& a = *(KArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  const Tile t = a.tiles[blockIdx.x];
  const float fac = a.tfac[blockIdx.x];
  const int base = t.kind & 0xFF, ls = (t.kind >> 8) & 0xFF;
  const int n = a.n;
  const bool inner = base == K_F32_TGPU_IN || base == K_I64_TGPU_IN;
  if constexpr (LS == 0) {
    if (base == K_F32_TGPU_W) {
      constexpr bool P = FA_TGPU16_S1_PASSES != 0;
      if (t.count == kTile) wide16<EL, 1, true, P, WIDE>(a, t.start, t.count, fac);
      else wide16<EL, 1, false, P, WIDE>(a, t.start, t.count, fac);
      return;
    }
  }
  if constexpr (LS == 1) {
    if (base == K_F32_TGPU_W) {
      constexpr bool P = FA_TGPU16_S2_PASSES != 0;
      if (ls == 0) {
        if (t.count == kTile) wide16<EL, 1, true, P, WIDE>(a, t.start, t.count, fac);
        else wide16<EL, 1, false, P, WIDE>(a, t.start, t.count, fac);
      } else {
        if (t.count == kTile) wide16<EL, 2, true, P, WIDE>(a, t.start, t.count, fac);
        else wide16<EL, 2, false, P, WIDE>(a, t.start, t.count, fac);
      }
      return;
    }
    if (!inner && ls != 1) {  // a rider: S = 1 or 4
      if (base == K_F32_TGPU_V) v_tile<EL, 4, WIDE>(a, t, fac);
      else if (ls == 0) scalar_tile<EL, 1, WIDE>(a, t, fac);
      else scalar_tile<EL, 4, WIDE>(a, t, fac);
      return;
    }
  }
  if (base == K_F32_TGPU_V) {
    if constexpr (S >= 4) v_tile<EL, S, WIDE>(a, t, fac);  // (S <= 2 keys make W tiles)
    return;
  }
  if (base == K_F32_TGPU || base == K_I64_TGPU) {
    scalar_tile<EL, S, WIDE>(a, t, fac);
    return;
  }
  if (!inner) return;
  // inner: one element per wave
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (w >= t.count) return;
  const int64_t e = t.start + w;
  const int bw = 1 << ls;
  const bool vec = (t.kind >> 16) & 1;  // N >= 128: input-vectorised form
  if (base == K_F32_TGPU_IN) {
    const float s = vec ? tgpu_inner_vec(Src16<EL>{a}, e, n, bw, lane)
                        : tgpu_inner(Src16<EL>{a}, e, n, bw, lane);
    if constexpr (WIDE) {
      if (lane == 0) a.out32[e] = __fmul_rn(s, fac);
    } else {
      if (lane == 0) ((uint16_t*)a.out32)[e] = (uint16_t)narrow<EL>(mean32(s, fac));
    }
  } else {
    const float s = vec ? tgpu_inner_vec(SrcI64{a}, e, n, bw, lane)
                        : tgpu_inner(SrcI64{a}, e, n, bw, lane);
    if (lane == 0) a.out64[e] = (int64_t)__fmul_rn(s, fac);
  }
}

template <int EL, bool WIDE>
static hipError_t launch_el(const ReduceArgs& a, int group, int ntiles, hipStream_t st) {
  const dim3 g(ntiles), b(kBlock);
  // no LDS reservation on the S = 2 launch: fedagg.hip's tgpu_s2_lds was
  // measured on the fp32 instance only
  switch (group) {
    case 0: hipLaunchKernelGGL((tgpu16_kernel<EL, 0, WIDE>), g, b, 0, st, a); break;
    case 1: hipLaunchKernelGGL((tgpu16_kernel<EL, 1, WIDE>), g, b, 0, st, a); break;
    case 2: hipLaunchKernelGGL((tgpu16_kernel<EL, 2, WIDE>), g, b, 0, st, a); break;
    case 3: hipLaunchKernelGGL((tgpu16_kernel<EL, 3, WIDE>), g, b, 0, st, a); break;
    case 4: hipLaunchKernelGGL((tgpu16_kernel<EL, 4, WIDE>), g, b, 0, st, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch(const ReduceArgs& a, int group, int ntiles, int elem, bool wide,
                  hipStream_t st) {
  if (ntiles <= 0) return hipSuccess;
  if (elem == FA_ELEM_F16)
    return wide ? launch_el<FA_ELEM_F16, true>(a, group, ntiles, st)
                : launch_el<FA_ELEM_F16, false>(a, group, ntiles, st);
  if (elem == FA_ELEM_BF16)
    return wide ? launch_el<FA_ELEM_BF16, true>(a, group, ntiles, st)
                : launch_el<FA_ELEM_BF16, false>(a, group, ntiles, st);
  return hipErrorInvalidValue;
}

template <bool WIDE>
static int occupancy_s1_w(int elem) {
  int occ = 0;
  const hipError_t e =
      elem == FA_ELEM_F16
          ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, tgpu16_kernel<FA_ELEM_F16, 0, WIDE>,
                                                         kBlock, 0)
          : hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, tgpu16_kernel<FA_ELEM_BF16, 0, WIDE>,
                                                         kBlock, 0);
  return e == hipSuccess ? occ : 0;
}

int occupancy_s1(int elem, bool wide) {
  return wide ? occupancy_s1_w<true>(elem) : occupancy_s1_w<false>(elem);
}

}  // namespace fa_tgpu16
