// prox_h16.hip — the FedProx proximal term (prox.hip) for fp16 / bf16 clients:
// model.half() / model.bfloat16() federations, whose parameters sit in 16-bit
// buckets (fedagg_h16.hip), the global in a 16-bit bucket ("pure") or in an
// fp32 master bucket at the same element offsets ("mixed").  The reference's
// line, per parameter,
//
//     proximal_term += (w - w_t).norm(2)
//
// as torch computes it for these dtypes on the CPU:
//
//   pure   d16 = rn16(fp32(w) - fp32(w_t)); the norm accumulates d16^2 in
//          fp32 (the order free, as in prox.hip), takes the square root and is
//          ROUNDED TO 16 BITS: n16[k]; the term is the running 16-bit sum of
//          the n16[k] in parameter order, run = rn16(run + n16[k]) from
//          n16[0]; grad_w = rn16(gout16 * rn16(d16 / n16[k])) (IEEE division
//          in fp32; 0 where n16[k] == 0), grad_w_t its negation, both 16-bit;
//          an accumulating side is rn16(fp32(old) + fp32(new)).
//   mixed  w - w_t promotes to fp32: prox.hip's arithmetic on fp32(w) (exact
//          widening), fp32 norms, total and global gradient; the client's
//          gradient is rn16 of the fp32 one (autograd casts it to its input's
//          dtype), an accumulating client side rn16(fp32(old) + fp32(that)).
//
// Every 16-bit rounding above is part of the definition; only the fp32
// sum-of-squares order is ours.  Launches as prox.hip's: partials (one
// workgroup per chunk of <= 4096 elements of one tensor, prox.hip's chunk
// table, element-based), a one-workgroup finish, one backward.  The pure
// finish rounds each norm to 16 bits and then ONE lane walks them in order
// with a narrowing after every add — the serial sum is torch's definition
// (in bf16, 256 followed by 64 ones is 256; reversed it is 320).  The mixed
// finish is prox.hip's fp32 one.
//
// Its own translation unit and kernel family: prox.hip's fp32 kernels are not
// templated on the element type (code a launch never runs costs the other
// instances).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"
#include "conv16.h"
#include "prox_plan.h"

namespace fa_prox16 {
using fa_h16::f4;
using fa_h16::narrow;
using fa_h16::narrow8;
using fa_h16::u4;
using fa_h16::widen;
using fa_h16::widen8;
using fa_prox::Chunk;

constexpr int kBlk = 256;
constexpr int kChunk = 4096;                 // elements per workgroup (prox.hip kChunk)
constexpr int kVec = 8;                      // elements per 16-B load of a 16-bit bucket
constexpr int kLoads = kChunk / (kVec * kBlk);  // 16-bit loads per lane: 2
constexpr int kFinBlk = 1024;
constexpr int kFinLoads = 8;

// Cache policy: prox.hip's choice — plain loads forward (the backward of a
// training step runs right after it and finds the buckets in the 256 MB MALL),
// non-temporal loads and stores backward.  Measured for 16-bit data (forward
// then backward on the same buckets, tools/prox16_ab.py pair):
// 27.4 us pure / 38.4 mixed, against 33.3 / 43.6 with non-temporal forward
// loads too and 34.9 / 43.8 with plain loads and stores throughout.  The
// macros are that A/B's knobs; the library ships the defaults.
#ifndef FA_PROX16_NT_LOAD_FWD
#define FA_PROX16_NT_LOAD_FWD 0
#endif
#ifndef FA_PROX16_NT_LOAD_BWD
#define FA_PROX16_NT_LOAD_BWD 1
#endif
#ifndef FA_PROX16_NT_STORE
#define FA_PROX16_NT_STORE 1
#endif
template <bool NT, class T>
__device__ __forceinline__ T ld(const T* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <class T>
__device__ __forceinline__ T ld_fwd(const T* p) { return ld<FA_PROX16_NT_LOAD_FWD != 0>(p); }
template <class T>
__device__ __forceinline__ T ld_nt(const T* p) { return ld<FA_PROX16_NT_LOAD_BWD != 0>(p); }
template <class T>
__device__ __forceinline__ void st_nt(T* p, T v) {
  if constexpr (FA_PROX16_NT_STORE != 0) __builtin_nontemporal_store(v, p);
  else *p = v;
}

__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// A value about to be narrowed, pinned in a register: with fp16 the compiler
// may otherwise fold the arithmetic that made it into a mixed-precision
// instruction (conv16.h widen's pin, on the other side of the conversion).
__device__ __forceinline__ float pin(float x) {
  asm volatile("" : "+v"(x));
  return x;
}
// rn16 as an fp32 value: narrowed and widened again.
template <int EL>
__device__ __forceinline__ float rq(float x) { return widen<EL>(narrow<EL>(pin(x))); }
template <int EL>
__device__ __forceinline__ f4 rq4(f4 v) {
  return f4{rq<EL>(v.x), rq<EL>(v.y), rq<EL>(v.z), rq<EL>(v.w)};
}
__device__ __forceinline__ f4 pin4(f4 v) { return f4{pin(v.x), pin(v.y), pin(v.z), pin(v.w)}; }
__device__ __forceinline__ float sq4(f4 d) { return d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w; }

// ------------------------------------------------------------- forward ----
// Lane t owns 16-bit vectors t and t + 256 of the chunk (8 elements each); in
// the mixed form the fp32 side's two 16-B loads per vector are 2v and 2v + 1
// (fedagg_h16.hip bcast_narrow_kernel's pairing).  All loads are issued before
// any arithmetic.  Chunk starts are multiples of 8 elements (the plan's
// align8): 16 B of the 16-bit bucket, 32 B of the fp32 one.  count % 8
// trailing elements go through the scalar tail.  Per lane the squares are
// added as in prox.hip — 3 adds inside each group of four, 1 into the
// accumulator, 4 groups: 16 in-lane adds — then the tail's add, the wave
// shuffles and thread 0's sum of the 4 waves.  PURE: every difference is
// rounded to 16 bits before it is squared (the square of a 16-bit value is
// exact in fp32); mixed: it is not.
template <int EL, bool MIXED>
__global__ __launch_bounds__(kBlk) void prox_partials16(const Chunk* __restrict__ chunks,
                                                        const uint16_t* __restrict__ a,
                                                        const void* __restrict__ bv,
                                                        float* __restrict__ partials) {
  __shared__ float lds[kBlk / 64];
  const Chunk c = chunks[blockIdx.x];
  const int nv = c.count / kVec;
  const u4* pa = reinterpret_cast<const u4*>(a + c.start);
  const u4 z4 = u4{0u, 0u, 0u, 0u};
  const f4 zf = f4{0.f, 0.f, 0.f, 0.f};
  u4 xa[kLoads];
  float acc = 0.f;
  if constexpr (MIXED) {
    const float* b = static_cast<const float*>(bv);
    const f4* pb = reinterpret_cast<const f4*>(b + c.start);
    f4 xb[kLoads][2];
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
      const int v = threadIdx.x + u * kBlk;
      const bool ok = v < nv;
      xa[u] = ok ? ld_fwd(pa + v) : z4;
      xb[u][0] = ok ? ld_fwd(pb + 2 * v) : zf;
      xb[u][1] = ok ? ld_fwd(pb + 2 * v + 1) : zf;
    }
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
      f4 a0, a1;
      widen8<EL>(xa[u], &a0, &a1);
      acc += sq4(a0 - xb[u][0]);
      acc += sq4(a1 - xb[u][1]);
    }
    for (int j = kVec * nv + threadIdx.x; j < c.count; j += kBlk) {
      const float d = widen<EL>(a[c.start + j]) - b[c.start + j];
      acc += d * d;
    }
  } else {
    const uint16_t* b = static_cast<const uint16_t*>(bv);
    const u4* pb = reinterpret_cast<const u4*>(b + c.start);
    u4 xb[kLoads];
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
      const int v = threadIdx.x + u * kBlk;
      const bool ok = v < nv;
      xa[u] = ok ? ld_fwd(pa + v) : z4;
      xb[u] = ok ? ld_fwd(pb + v) : z4;
    }
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
      f4 a0, a1, b0, b1;
      widen8<EL>(xa[u], &a0, &a1);
      widen8<EL>(xb[u], &b0, &b1);
      acc += sq4(rq4<EL>(a0 - b0));
      acc += sq4(rq4<EL>(a1 - b1));
    }
    for (int j = kVec * nv + threadIdx.x; j < c.count; j += kBlk) {
      const float d = rq<EL>(widen<EL>(a[c.start + j]) - widen<EL>(b[c.start + j]));
      acc += d * d;
    }
  }
  acc = wave_sum(acc);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0) lds[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float r = 0.f;
    for (int i = 0; i < kBlk / 64; ++i) r += lds[i];
    partials[blockIdx.x] = r;
  }
}

// ---------------------------------------------------------- pure finish ----
// prox.hip's finish (one workgroup; the partials and the segment boundaries
// staged in LDS with one round of independent loads when they fit, else read
// from global memory in the same order; wave w sums tensors w, w + W, ...:
// lane l partials l, l + 64, ..., then the shuffle tree) with the two 16-bit
// steps of the definition: norms[k] = rn16(sqrt(sum)), stored widened, and
// the total as ONE lane's in-order walk over the norms with a narrowing
// after every add.  An empty plan's total is +0.
template <int EL, bool LDS>
__global__ __launch_bounds__(kFinBlk) void prox_finish16(const int* __restrict__ seg_first,
                                                         int nseg, int nchunks,
                                                         const float* __restrict__ partials,
                                                         float* __restrict__ norms,
                                                         uint16_t* __restrict__ total) {
  extern __shared__ float dyn[];
  // LDS: [nchunks partials][nseg + 1 boundaries][nseg norms]
  const float* P = partials;
  const int* F = seg_first;
  float* NL = norms;
  if constexpr (LDS) {
    float* sp = dyn;
    int* sf = reinterpret_cast<int*>(dyn + nchunks);
    const int f0 = (int)threadIdx.x <= nseg ? seg_first[threadIdx.x] : 0;
    for (int base = 0; base < nchunks; base += kFinBlk * kFinLoads) {
      float x[kFinLoads];
#pragma unroll
      for (int i = 0; i < kFinLoads; ++i) {
        const int j = base + threadIdx.x + i * kFinBlk;
        x[i] = j < nchunks ? partials[j] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < kFinLoads; ++i) {
        const int j = base + threadIdx.x + i * kFinBlk;
        if (j < nchunks) sp[j] = x[i];
      }
    }
    if ((int)threadIdx.x <= nseg) sf[threadIdx.x] = f0;
    for (int j = threadIdx.x + kFinBlk; j <= nseg; j += kFinBlk) sf[j] = seg_first[j];
    __syncthreads();
    P = sp;
    F = sf;
    NL = reinterpret_cast<float*>(sf + nseg + 1);
  }
  constexpr int kWaves = kFinBlk / 64;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int k = wave; k < nseg; k += kWaves) {
    float sq = 0.f;
    for (int i = F[k] + lane; i < F[k + 1]; i += 64) sq += P[i];
    sq = wave_sum(sq);
    if (lane == 0) {
      const float n = rq<EL>(sqrtf(sq));
      norms[k] = n;
      if constexpr (LDS) NL[k] = n;
    }
  }
  __syncthreads();  // the norms written by this workgroup's waves
  if (threadIdx.x == 0) {
    float run = nseg > 0 ? NL[0] : 0.f;
    for (int k = 1; k < nseg; ++k) run = rq<EL>(run + NL[k]);
    *total = (uint16_t)narrow<EL>(run);
  }
}

// ------------------------------------------------------------ backward ----
// Per chunk both sides are read (non-temporal) and grad_a is written in the
// client's type, grad_b — when given — in the global's.  ACC / ACCB: that
// side is added to what its bucket holds, in its own type.  Only elements
// inside segments are written.
//
// PURE: one element's gradient, as 16 bits.
template <int EL>
__device__ __forceinline__ uint32_t grad16(float af, float bf, float nk, float gs, bool zero) {
  const float d = rq<EL>(af - bf);
  const float q = rq<EL>(__fdiv_rn(d, nk));
  return zero ? 0u : narrow<EL>(pin(gs * q));
}
template <int EL>
__device__ __forceinline__ u4 grad16x8(f4 a0, f4 a1, f4 b0, f4 b1, float nk, float gs, bool zero) {
  uint32_t g[8];
  g[0] = grad16<EL>(a0.x, b0.x, nk, gs, zero);
  g[1] = grad16<EL>(a0.y, b0.y, nk, gs, zero);
  g[2] = grad16<EL>(a0.z, b0.z, nk, gs, zero);
  g[3] = grad16<EL>(a0.w, b0.w, nk, gs, zero);
  g[4] = grad16<EL>(a1.x, b1.x, nk, gs, zero);
  g[5] = grad16<EL>(a1.y, b1.y, nk, gs, zero);
  g[6] = grad16<EL>(a1.z, b1.z, nk, gs, zero);
  g[7] = grad16<EL>(a1.w, b1.w, nk, gs, zero);
  return u4{g[0] | (g[1] << 16), g[2] | (g[3] << 16), g[4] | (g[5] << 16), g[6] | (g[7] << 16)};
}
// AccumulateGrad in 16 bits: rn16(fp32(old) + fp32(new)), 8 elements.
template <int EL>
__device__ __forceinline__ u4 acc16x8(u4 old, u4 g) {
  f4 o0, o1, g0, g1;
  widen8<EL>(old, &o0, &o1);
  widen8<EL>(g, &g0, &g1);
  return narrow8<EL>(pin4(o0 + g0), pin4(o1 + g1));
}
template <int EL>
__device__ __forceinline__ uint16_t acc16(uint16_t old, uint32_t g) {
  return (uint16_t)narrow<EL>(pin(widen<EL>(old) + widen<EL>(g)));
}
__device__ __forceinline__ u4 neg8(u4 g) {  // the sign bit of all 8 elements flipped
  const uint32_t m = 0x80008000u;
  return u4{g.x ^ m, g.y ^ m, g.z ^ m, g.w ^ m};
}

template <int EL, bool ACC, bool ACCB>
__global__ __launch_bounds__(kBlk) void prox_grad16(const Chunk* __restrict__ chunks,
                                                    const uint16_t* __restrict__ a,
                                                    const uint16_t* __restrict__ b,
                                                    const float* __restrict__ norms,
                                                    const uint16_t* __restrict__ gout, float alpha,
                                                    uint16_t* __restrict__ ga,
                                                    uint16_t* __restrict__ gb) {
  const Chunk c = chunks[blockIdx.x];
  const float nk = norms[c.seg];
  // the scale rn16(gout * alpha); only a zero norm is masked (torch's norm
  // backward): a NaN norm gives NaNs for its whole tensor, an infinite one
  // (fp16 overflow) zeros
  const float gs = rq<EL>(widen<EL>(*gout) * alpha);
  const bool zero = nk == 0.f;
  const int nv = c.count / kVec;
  const u4* pa = reinterpret_cast<const u4*>(a + c.start);
  const u4* pb = reinterpret_cast<const u4*>(b + c.start);
  u4* qa = reinterpret_cast<u4*>(ga + c.start);
  u4* qb = reinterpret_cast<u4*>(gb + c.start);
  const u4 z4 = u4{0u, 0u, 0u, 0u};
  u4 xa[kLoads], xb[kLoads];
#pragma unroll
  for (int u = 0; u < kLoads; ++u) {
    const int v = threadIdx.x + u * kBlk;
    const bool ok = v < nv;
    xa[u] = ok ? ld_nt(pa + v) : z4;
    xb[u] = ok ? ld_nt(pb + v) : z4;
  }
#pragma unroll
  for (int u = 0; u < kLoads; ++u) {
    const int v = threadIdx.x + u * kBlk;
    if (v < nv) {
      f4 a0, a1, b0, b1;
      widen8<EL>(xa[u], &a0, &a1);
      widen8<EL>(xb[u], &b0, &b1);
      const u4 g = grad16x8<EL>(a0, a1, b0, b1, nk, gs, zero);
      if constexpr (ACC) st_nt(qa + v, acc16x8<EL>(ld_nt(qa + v), g));
      else st_nt(qa + v, g);
      if (gb) {
        if constexpr (ACCB) st_nt(qb + v, acc16x8<EL>(ld_nt(qb + v), neg8(g)));
        else st_nt(qb + v, neg8(g));
      }
    }
  }
  for (int j = kVec * nv + threadIdx.x; j < c.count; j += kBlk) {
    const int64_t e = c.start + j;
    const uint32_t g = grad16<EL>(widen<EL>(a[e]), widen<EL>(b[e]), nk, gs, zero);
    ga[e] = ACC ? acc16<EL>(ga[e], g) : (uint16_t)g;
    if (gb) gb[e] = ACCB ? acc16<EL>(gb[e], g ^ 0x8000u) : (uint16_t)(g ^ 0x8000u);
  }
}

// MIXED: prox.hip's fp32 gradient d = g * (fp32(a) - b), g = gout * alpha /
// norms[k]; grad_b = -d (ACCB: grad_b - d) in fp32, grad_a = rn16(d) (ACC:
// rn16(fp32(old) + fp32(rn16(d)))).
template <int EL, bool ACC, bool ACCB>
__global__ __launch_bounds__(kBlk) void prox_grad16m(const Chunk* __restrict__ chunks,
                                                     const uint16_t* __restrict__ a,
                                                     const float* __restrict__ b,
                                                     const float* __restrict__ norms,
                                                     const float* __restrict__ gout, float alpha,
                                                     uint16_t* __restrict__ ga,
                                                     float* __restrict__ gb) {
  const Chunk c = chunks[blockIdx.x];
  const float nk = norms[c.seg];
  const float g = nk == 0.f ? 0.f : (*gout) * alpha / nk;
  const int nv = c.count / kVec;
  const u4* pa = reinterpret_cast<const u4*>(a + c.start);
  const f4* pb = reinterpret_cast<const f4*>(b + c.start);
  u4* qa = reinterpret_cast<u4*>(ga + c.start);
  f4* qb = reinterpret_cast<f4*>(gb + c.start);
  const u4 z4 = u4{0u, 0u, 0u, 0u};
  const f4 zf = f4{0.f, 0.f, 0.f, 0.f};
  u4 xa[kLoads];
  f4 xb[kLoads][2];
#pragma unroll
  for (int u = 0; u < kLoads; ++u) {
    const int v = threadIdx.x + u * kBlk;
    const bool ok = v < nv;
    xa[u] = ok ? ld_nt(pa + v) : z4;
    xb[u][0] = ok ? ld_nt(pb + 2 * v) : zf;
    xb[u][1] = ok ? ld_nt(pb + 2 * v + 1) : zf;
  }
#pragma unroll
  for (int u = 0; u < kLoads; ++u) {
    const int v = threadIdx.x + u * kBlk;
    if (v < nv) {
      f4 a0, a1;
      widen8<EL>(xa[u], &a0, &a1);
      const f4 d0 = g * (a0 - xb[u][0]), d1 = g * (a1 - xb[u][1]);
      const u4 r = narrow8<EL>(pin4(d0), pin4(d1));
      if constexpr (ACC) st_nt(qa + v, acc16x8<EL>(ld_nt(qa + v), r));
      else st_nt(qa + v, r);
      if (gb) {
        if constexpr (ACCB) {
          st_nt(qb + 2 * v, ld_nt(qb + 2 * v) - d0);
          st_nt(qb + 2 * v + 1, ld_nt(qb + 2 * v + 1) - d1);
        } else {
          st_nt(qb + 2 * v, -d0);
          st_nt(qb + 2 * v + 1, -d1);
        }
      }
    }
  }
  for (int j = kVec * nv + threadIdx.x; j < c.count; j += kBlk) {
    const int64_t e = c.start + j;
    const float d = g * (widen<EL>(a[e]) - b[e]);
    const uint32_t r = narrow<EL>(pin(d));
    ga[e] = ACC ? acc16<EL>(ga[e], r) : (uint16_t)r;
    if (gb) gb[e] = ACCB ? gb[e] - d : -d;
  }
}

// --------------------------------------------------------------- launch ----
template <int EL>
static hipError_t norms_el(const fa_norm_plan* p, const fa_prox::PlanView& v, const void* a,
                           const void* b, bool mixed, float* norms, void* total, hipStream_t st) {
  if (v.nchunks > 0) {
    if (mixed)
      hipLaunchKernelGGL((prox_partials16<EL, true>), dim3(v.nchunks), dim3(kBlk), 0, st,
                         v.d_chunks, (const uint16_t*)a, b, v.d_partials);
    else
      hipLaunchKernelGGL((prox_partials16<EL, false>), dim3(v.nchunks), dim3(kBlk), 0, st,
                         v.d_chunks, (const uint16_t*)a, b, v.d_partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (mixed) return fa_prox::launch_finish_f32(p, norms, (float*)total, st);
  const size_t lds = fa_prox::finish_lds_bytes(p);
  if (lds)
    hipLaunchKernelGGL((prox_finish16<EL, true>), dim3(1), dim3(kFinBlk), lds, st, v.d_seg_first,
                       v.nseg, v.nchunks, v.d_partials, norms, (uint16_t*)total);
  else
    hipLaunchKernelGGL((prox_finish16<EL, false>), dim3(1), dim3(kFinBlk), 0, st, v.d_seg_first,
                       v.nseg, v.nchunks, v.d_partials, norms, (uint16_t*)total);
  return hipGetLastError();
}

template <int EL>
static hipError_t grad_el(const fa_prox::PlanView& v, const void* a, const void* b, bool mixed,
                          const float* norms, const void* gout, float alpha, void* ga, void* gb,
                          bool acc_a, bool acc_b, hipStream_t st) {
  if (mixed) {
    auto k = acc_a ? (acc_b ? prox_grad16m<EL, true, true> : prox_grad16m<EL, true, false>)
                   : (acc_b ? prox_grad16m<EL, false, true> : prox_grad16m<EL, false, false>);
    hipLaunchKernelGGL(k, dim3(v.nchunks), dim3(kBlk), 0, st, v.d_chunks, (const uint16_t*)a,
                       (const float*)b, norms, (const float*)gout, alpha, (uint16_t*)ga,
                       (float*)gb);
  } else {
    auto k = acc_a ? (acc_b ? prox_grad16<EL, true, true> : prox_grad16<EL, true, false>)
                   : (acc_b ? prox_grad16<EL, false, true> : prox_grad16<EL, false, false>);
    hipLaunchKernelGGL(k, dim3(v.nchunks), dim3(kBlk), 0, st, v.d_chunks, (const uint16_t*)a,
                       (const uint16_t*)b, norms, (const uint16_t*)gout, alpha, (uint16_t*)ga,
                       (uint16_t*)gb);
  }
  return hipGetLastError();
}

// 0: (F32, F32); 1: pure 16-bit; 2: mixed; -1: not supported
static int pair_form(int a_elem, int b_elem) {
  if (a_elem == FA_ELEM_F32 && b_elem == FA_ELEM_F32) return 0;
  if (a_elem != FA_ELEM_F16 && a_elem != FA_ELEM_BF16) return -1;
  if (b_elem == a_elem) return 1;
  if (b_elem == FA_ELEM_F32) return 2;
  return -1;
}

}  // namespace fa_prox16

#define FA_PROX_PAIRS "(F16, F16), (BF16, BF16), (F16, F32), (BF16, F32) and (F32, F32)"

extern "C" {

int fa_prox_norms_elem(const fa_norm_plan* p, const void* a, int a_elem, const void* b, int b_elem,
                       float* norms, void* total, void* stream) {
  const int form = fa_prox16::pair_form(a_elem, b_elem);
  if (form < 0)
    return fa::set_err(FA_E_INVAL, "fa_prox_norms_elem: element pair (%d, %d) not supported: "
                       FA_PROX_PAIRS " are", a_elem, b_elem);
  if (form == 0)
    return fa_prox_norms(p, (const float*)a, (const float*)b, norms, (float*)total, stream);
  if (!p || !a || !b || !norms || !total)
    return fa::set_err(FA_E_INVAL, "fa_prox_norms_elem: NULL argument");
  const fa_prox::PlanView v = fa_prox::view(p);
  if (!v.align8)
    return fa::set_err(FA_E_ALIGN, "fa_prox_norms_elem: a 16-bit bucket needs every segment "
                       "offset to be a multiple of 8 elements");
  if (((uintptr_t)a | (uintptr_t)b) & 15u)
    return fa::set_err(FA_E_ALIGN, "fa_prox_norms_elem: buckets must be 16-B aligned");
  const hipError_t e =
      a_elem == FA_ELEM_F16
          ? fa_prox16::norms_el<FA_ELEM_F16>(p, v, a, b, form == 2, norms, total, (hipStream_t)stream)
          : fa_prox16::norms_el<FA_ELEM_BF16>(p, v, a, b, form == 2, norms, total, (hipStream_t)stream);
  FA_HIP_TRY(e);
  return FA_OK;
}

int fa_prox_grad_elem(const fa_norm_plan* p, const void* a, int a_elem, const void* b, int b_elem,
                      const float* norms, const void* gout, float alpha, void* grad_a,
                      void* grad_b, unsigned flags, void* stream) {
  const int form = fa_prox16::pair_form(a_elem, b_elem);
  if (form < 0)
    return fa::set_err(FA_E_INVAL, "fa_prox_grad_elem: element pair (%d, %d) not supported: "
                       FA_PROX_PAIRS " are", a_elem, b_elem);
  if (form == 0)
    return fa_prox_grad_ex(p, (const float*)a, (const float*)b, norms, (const float*)gout, alpha,
                           (float*)grad_a, (float*)grad_b, flags, stream);
  if (!p || !a || !b || !norms || !gout || !grad_a)
    return fa::set_err(FA_E_INVAL, "fa_prox_grad_elem: NULL argument");
  if (flags & ~(FA_PROX_ACCUMULATE | FA_PROX_ACCUMULATE_A | FA_PROX_ACCUMULATE_B))
    return fa::set_err(FA_E_INVAL, "fa_prox_grad_elem: bad flags");
  const fa_prox::PlanView v = fa_prox::view(p);
  if (!v.align8)
    return fa::set_err(FA_E_ALIGN, "fa_prox_grad_elem: a 16-bit bucket needs every segment "
                       "offset to be a multiple of 8 elements");
  if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)grad_a | (uintptr_t)grad_b) & 15u)
    return fa::set_err(FA_E_ALIGN, "fa_prox_grad_elem: buckets must be 16-B aligned");
  if (v.nchunks == 0) return FA_OK;
  const bool acc_a = flags & (FA_PROX_ACCUMULATE | FA_PROX_ACCUMULATE_A);
  const bool acc_b = flags & (FA_PROX_ACCUMULATE | FA_PROX_ACCUMULATE_B);
  const hipError_t e =
      a_elem == FA_ELEM_F16
          ? fa_prox16::grad_el<FA_ELEM_F16>(v, a, b, form == 2, norms, gout, alpha, grad_a, grad_b,
                                            acc_a, acc_b, (hipStream_t)stream)
          : fa_prox16::grad_el<FA_ELEM_BF16>(v, a, b, form == 2, norms, gout, alpha, grad_a, grad_b,
                                             acc_a, acc_b, (hipStream_t)stream);
  FA_HIP_TRY(e);
  return FA_OK;
}

}  // extern "C"
