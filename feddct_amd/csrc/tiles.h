// tiles.h — the tile table's types and the constants its planners and
// kernels share.  No HIP: included by the host planners (plan_host.cpp, plain
// C++) and, through reduce_impl.h, by every kernel unit.
#pragma once
#include <cstdint>

#ifdef __HIP__
#define FA_HOST_DEVICE __host__ __device__
#else
#define FA_HOST_DEVICE
#endif

namespace fa_k {

// ----------------------------------------------------------------- tiles --
enum TileKind : int32_t {
  K_F32_VEC = 0,      // cascade order, 16-B vectors, count % 4 == 0
  K_F32_CASC_S = 1,   // cascade order, one element per thread (unaligned)
  K_F32_ILP4 = 2,     // tail columns: ILP-4 order
  K_F32_INNER = 3,    // M == 1: ILP-4 (n < 8) or 8-lane inner (n >= 8)
  K_I64_CASC = 4,
  K_I64_ILP4 = 5,
  K_I64_INNER = 6,
  // torch-ROCm's GPU order (fa_plan_create_order, FA_ORDER_TORCH_GPU); the
  // tile's kind carries log2 of its stride in bits 8-15
  K_F32_TGPU = 7,     // [N, M>=2]: S-way row split, 4 round-robin accumulators
  K_I64_TGPU = 8,
  K_F32_TGPU_IN = 9,  // M == 1: lane split + intra-wave shuffle tree, 1 element/wave
  K_I64_TGPU_IN = 10,
  K_F32_TGPU_V = 11,  // [N, M>=2], 16-B aligned run: 4 elements per lane, up to 1024
  K_F32_TGPU_W = 12,  // the same with S = 1: 8 elements per lane (2 x 16 B), up to 2048
  // device tables only (r03): the plan's scalar tiles (kinds 1-6) packed,
  // up to 256 elements of any tensors per tile; `start` indexes the plan's
  // scalar index, whose entries are (bucket element << 4) | kind
  K_SCALAR_PACKED = 13,
};

FA_HOST_DEVICE inline bool kind_is64(int kind) {
  const int b = kind & 0xFF;
  return b == K_I64_CASC || b == K_I64_ILP4 || b == K_I64_INNER || b == K_I64_TGPU ||
         b == K_I64_TGPU_IN;
}

struct Tile {
  int64_t start;  // first element (bucket index)
  int32_t count;  // elements
  int32_t kind;
};
static_assert(sizeof(Tile) == 16, "tile is 16 B");

constexpr int kBlock = 256;
constexpr int kDefaultU = 2;
// MI355X's device properties as torch-ROCm's setReduceConfig reads them
// (multiProcessorCount, maxThreadsPerMultiProcessor): they decide where torch
// splits a reduction across blocks (fa_torch_gpu_config); a GPU test checks
// them against torch.cuda.get_device_properties.
constexpr int64_t kTorchNumCU = 256;
constexpr int64_t kTorchMaxThreadsPerCU = 2048;  // float4 vectors per thread per client (tools/tune.py)

// Columns of a packed scalar tile (K_SCALAR_PACKED; reduce_impl.h
// tile_scalar_packed): one per lane of wave 0.
constexpr int kPackCols = 64;

// c10::utils::CeilLog2 / ATen multi_row_sum level power: the cascade's level
// step for n rows, read by the kernels and by the host's chain levels alike
FA_HOST_DEVICE inline int ceil_log2_i(int64_t n) {
  if (n <= 1) return 0;
  int r = 0;
  uint64_t v = (uint64_t)(n - 1);
  while (v) { ++r; v >>= 1; }
  return r;
}
FA_HOST_DEVICE inline int level_power(int64_t n) {
  int c = ceil_log2_i(n) / 4;
  return c > 4 ? c : 4;
}

}  // namespace fa_k

namespace fa_h16 {
// Elements of a 16-bit vector tile per 16-B load per lane of the 256-thread
// workgroup: a tile is u * kTile elements, u in {1, 2}.
constexpr int kVec = 8;
constexpr int kTile = kVec * fa_k::kBlock;  // 2048
constexpr int kDefaultU = 1;                // 2048-element tiles: measured, DESIGN §4.8
}  // namespace fa_h16
