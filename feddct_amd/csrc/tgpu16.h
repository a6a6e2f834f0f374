// tgpu16.h — launcher of the torch-GPU-order reduce over fp16 / bf16 buckets
// (fedagg_tgpu16.hip), called by fedagg.hip's fa_reduce_tab for plans made by
// fa_plan_create_order_elem with a 16-bit element type, and by
// fa_plan_create_order_elem_out (an fp32 result bucket).
#pragma once
#include <hip/hip_runtime.h>

#include "reduce_impl.h"

namespace fa_tgpu16 {
// One workgroup per tile of the launch group `group` (row split S = 1 <<
// group; the plan's tg_lo[group] .. tg_lo[group + 1]) whose tiles, factors
// and count are in `a`.  `a.c32[]` / `a.tab32[]` carry the 16-bit bucket
// pointers; `a.out32` the 16-bit result bucket, or with `wide` an fp32 bucket
// that takes the unrounded fp32 result at the same element offsets.
hipError_t launch(const fa_k::ReduceArgs& a, int group, int ntiles, int elem, bool wide,
                  hipStream_t st);

// Workgroups of the S = 1 group's kernel a CU holds (0: the query failed).
int occupancy_s1(int elem, bool wide);
}  // namespace fa_tgpu16
