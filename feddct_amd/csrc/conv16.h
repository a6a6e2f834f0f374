// conv16.h — the fp16 / bf16 <-> fp32 conversions of the 16-bit kernels
// (fedagg_h16.hip's reduce and narrowing broadcast, prox_h16.hip's proximal
// term): one definition of "widen exactly" and "round to nearest-even as
// torch's CPU copy_" for every unit that reads or writes a 16-bit bucket.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/fedagg.h"

namespace fa_h16 {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------ conversions --
// Exact widening.  bf16 is the upper half of an fp32.  fp16: v_cvt_f32_f16
// (subnormals kept: the kernels run with the default denormal mode); the
// empty asm pins the converted value in a register, so the compiler cannot
// fold the conversion into a mixed-precision multiply-add.
template <int EL>
__device__ __forceinline__ float widen(uint32_t h) {  // h: the 16 bits, zero-extended
  if constexpr (EL == FA_ELEM_BF16) {
    return __uint_as_float(h << 16);
  } else {
    float f = (float)__builtin_bit_cast(_Float16, (uint16_t)h);
    asm volatile("" : "+v"(f));
    return f;
  }
}
// The two elements of one dword, low address first.
template <int EL>
__device__ __forceinline__ void widen2(uint32_t w, float* lo, float* hi) {
  if constexpr (EL == FA_ELEM_BF16) {
    *lo = __uint_as_float(w << 16);
    *hi = __uint_as_float(w & 0xffff0000u);
  } else {
    *lo = widen<EL>(w & 0xffffu);
    *hi = widen<EL>(w >> 16);
  }
}

// fp32 -> 16 bits, round to nearest-even, as torch's CPU copy_ (c10's
// round_to_nearest_even for bf16, the IEEE conversion for fp16: overflow to
// +-inf, subnormal results kept).  A NaN gives a quiet NaN.
template <int EL>
__device__ __forceinline__ uint32_t narrow(float x) {
  if constexpr (EL == FA_ELEM_BF16) {
    const uint32_t u = __float_as_uint(x);
    if (x != x) return 0x7fc0u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
  } else {
    return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)x);
  }
}
template <int EL>
__device__ __forceinline__ uint32_t narrow2(float lo, float hi) {
  return narrow<EL>(lo) | (narrow<EL>(hi) << 16);
}

template <int EL>
__device__ __forceinline__ void widen8(u4 v, f4* a, f4* b) {
  float f[8];
  widen2<EL>(v.x, &f[0], &f[1]);
  widen2<EL>(v.y, &f[2], &f[3]);
  widen2<EL>(v.z, &f[4], &f[5]);
  widen2<EL>(v.w, &f[6], &f[7]);
  *a = f4{f[0], f[1], f[2], f[3]};
  *b = f4{f[4], f[5], f[6], f[7]};
}
template <int EL>
__device__ __forceinline__ u4 narrow8(f4 lo, f4 hi) {
  return u4{narrow2<EL>(lo.x, lo.y), narrow2<EL>(lo.z, lo.w), narrow2<EL>(hi.x, hi.y),
            narrow2<EL>(hi.z, hi.w)};
}

}  // namespace fa_h16
