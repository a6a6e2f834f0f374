// h16.h — launcher of the 16-bit reduce kernels (fedagg_h16.hip), called by
// fedagg.hip's fa_reduce_tab for plans whose floating bucket holds fp16 or
// bf16 elements (fa_plan_create_elem), and of the narrowing broadcast of a
// mixed plan (fa_plan_create_elem_out: fp32 result, 16-bit clients).
#pragma once
#include <hip/hip_runtime.h>

#include "reduce_impl.h"

namespace fa_h16 {
// (kVec, kTile, kDefaultU — the 16-bit tile widths — are in tiles.h)

// One workgroup per tile of the table in `a` (packed scalar tiles first).
// `a.c32[]` / `a.tab32[]` / `a.out32` carry the 16-bit bucket pointers.
// `wide`: a.out32 is an fp32 bucket at the same element offsets and takes the
// fp32 mean unrounded (a mixed plan).
hipError_t launch(const fa_k::ReduceArgs& a, int ntiles, int elem, int u, bool weighted, bool wide,
                  hipStream_t st);

// Clients per workgroup of the narrowing broadcast (fedagg.hip kBcastGroupMax).
constexpr int kBcastGroup = 24;
// a.out32's fp32 bucket over [0, f32_numel) rounded to nearest-even into every
// client's 16-bit bucket (a.c32[] / a.tab32[]), a.out64's i64_numel elements
// copied into every int64 bucket; either count may be 0.
hipError_t bcast_narrow(const fa_k::ReduceArgs& a, int n, int elem, int64_t f32_numel,
                        int64_t i64_numel, hipStream_t st);

// src[0, numel) rounded to nearest-even into the one 16-bit bucket dst[0, numel)
// (fa_narrow_f32): both 16-B aligned, any numel.
hipError_t narrow_range(const float* src, void* dst, int elem, int64_t numel, hipStream_t st);
}  // namespace fa_h16

namespace fa_chain16 {
// A chain segment over 16-bit buckets (fedagg_chain16.hip), one workgroup per
// vector tile of the table in `a`: rows a.row0 .. a.row0 + a.n - 1 of an
// a.n_total-row reduction, from the fp32 state planes a.st_in / a.lev_in to
// a.st_out / a.lev_out, or (a.st_out NULL) finished into a.out32 — the 16-bit
// bucket, or with `wide` the fp32 one.
hipError_t launch(const fa_k::ReduceArgs& a, int ntiles, int elem, int u, bool weighted, bool wide,
                  hipStream_t st);
}  // namespace fa_chain16
