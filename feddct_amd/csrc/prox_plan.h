// prox_plan.h — what prox_h16.hip (the 16-bit proximal term) needs of a norm
// plan, which prox.hip owns: the chunk table, the partials' scratch and the
// fp32 finish.  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/fedagg.h"

namespace fa_prox {

// One chunk of the table: <= 4096 elements of ONE segment (prox.hip
// NormChunk's layout; element-based, so it serves every element type).
struct Chunk {
  int64_t start;
  int32_t count;
  int32_t seg;
};

struct PlanView {
  int nseg, nchunks;
  const Chunk* d_chunks;
  const int* d_seg_first;
  float* d_partials;
  bool align8;  // every segment offset a multiple of 8 elements (16 B of a 16-bit bucket)
};
PlanView view(const fa_norm_plan* p);

// The finish's size rule: partials, boundaries and norms staged in LDS when
// they fit the default dynamic-LDS limit (bytes; 0: read from global memory).
size_t finish_lds_bytes(const fa_norm_plan* p);

// prox.hip's fp32 finish over the plan's partials (fa_prox_norms' second
// launch): per segment sqrt of its chunk partials' sum -> norms[k], their
// sum -> total.
hipError_t launch_finish_f32(const fa_norm_plan* p, float* norms, float* total, hipStream_t st);

}  // namespace fa_prox
