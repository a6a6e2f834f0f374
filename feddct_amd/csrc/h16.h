// h16.h — launcher of the 16-bit reduce kernels (fedagg_h16.hip), called by
// fedagg.hip's fa_reduce_tab for plans whose floating bucket holds fp16 or
// bf16 elements (fa_plan_create_elem).
#pragma once
#include <hip/hip_runtime.h>

#include "reduce_impl.h"

namespace fa_h16 {
// Elements of a vector tile per 16-B load per lane of the 256-thread
// workgroup: a tile is u * kTile elements, u in {1, 2}.
constexpr int kVec = 8;
constexpr int kTile = kVec * fa_k::kBlock;  // 2048
constexpr int kDefaultU = 1;                // 2048-element tiles: measured, DESIGN §4.8

// One workgroup per tile of the table in `a` (packed scalar tiles first).
// `a.c32[]` / `a.tab32[]` / `a.out32` carry the 16-bit bucket pointers.
hipError_t launch(const fa_k::ReduceArgs& a, int ntiles, int elem, int u, bool weighted,
                  hipStream_t st);
}  // namespace fa_h16
