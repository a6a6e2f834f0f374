// sched_host.h — everything a multi-GPU round's schedule or modelled time
// depends on (libfedagg_comm.so): the geometry of a layout cut over the
// ranks, the per-rank operation lists of the four round forms, the stream
// rules the executor and the cost model both read, and the cost model.  Host
// arithmetic on integers and doubles: no HIP, no RCCL (sched_host.cpp is
// compiled as plain C++ and runs without a device or a communicator).
// fedcomm.hip owns the kernels, the plans' device resources, the executor,
// graph capture and the RCCL-facing C ABI; the host-only entry points
// (fa_describe_round[_elem], fa_round_model[_elem], fa_model_constants,
// fa_multi_select*) are defined in sched_host.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/fedagg_comm.h"
#include "err.h"

// (hidden: the library exports its C ABI only)
namespace fa_sched __attribute__((visibility("hidden"))) {

// ------------------------------------------------------------- geometry ----
struct Geo {
  int nranks = 1, rank = 0;
  std::vector<int> counts, first;  // per rank: slots held, first slot
  int n_total = 0, n_local = 0, lo_slot = 0, nmax = 0;
  int64_t f32_numel = 0, i64_numel = 0;
  unsigned flags = 0;
  int elem = FA_ELEM_F32;  // the floating bucket's element type (FA_ELEM_*)
  // floating tiles sorted by start (fp32, or 16-bit: in 16-bit elements, vector
  // tiles on 8-element boundaries); int64 tiles
  std::vector<fa_tile_desc> t32, t64;
};

// Bytes per element of the floating bucket; elements per 256 B of it, where
// cut_tiles may cut (64 fp32, 128 fp16 / bf16: partition.cut_align).
inline int elem_size(int elem) { return elem == FA_ELEM_F32 ? 4 : 2; }
inline int cut_align(int elem) { return 256 / elem_size(elem); }

// Chained: state hops rank to rank, chunk by chunk.
struct ChainGeo {
  std::vector<std::pair<int64_t, int64_t>> range;  // vector-tile chunks [lo, hi)
  int finisher = 0;                                // last rank holding clients
  unsigned lev_in = 0, lev_out = 0;
  int64_t t32_width = 0;                           // scalar fp32 columns
  int64_t t32_row = 0;                             // their stack row stride (64-aligned)
};

// Blocked mode geometry (the same on every rank).  Pieces are the cascade's
// blocks of 2^lp slots (0..K-1) and the remainder block (K, when
// n_total % 2^lp); a piece's slots lie on its starter and holder ranks.
struct BlockGeo {
  int lp = 4;
  int K = 0, P = 0;                       // complete blocks, pieces (K + remainder)
  std::vector<int> s0, s1;                // piece rows [s0, s1)
  std::vector<int> starter, holder;       // first / last row's rank
  std::vector<int> bsum_slot;             // local pieces: BSUM index on the holder (-1: spans)
  std::vector<int> plane;                 // spanning complete blocks: CONT plane of the sum
  int tail_piece = -1, head_piece = -1;   // this rank's spanning piece it starts / ends
  int nbsum = 0;                          // local pieces of this rank
  std::vector<int64_t> slo, shi;          // owner column stripes (vector tiles)
  int64_t row = 0;                        // stripe row stride (floats, 64-aligned)
};

// What one rank's schedule of a round depends on.
struct RoundGeo {
  int mode = 0;  // FA_MODE_*
  int xchg = 0;
  int req_chunks = 0;  // the column chunk count the round was built for
  Geo g;
  // e1: the chunks' ranges; chained / blocked: the vector-tile chunks' ranges
  std::vector<std::pair<int64_t, int64_t>> range;
  // e2 (r06: every stripe cut into nchunks column chunks)
  std::vector<int64_t> lo;                // nranks + 1 stripe bounds
  std::vector<std::vector<int64_t>> clo;  // per rank: nchunks + 1 chunk bounds
  int nchunks = 0;
  ChainGeo cg;
  BlockGeo bg;
};

// The striped round's default column chunks per stripe (fa_stripe_plan_create,
// nchunks 0): the chunk c + 1 exchange overlaps chunk c's stripe reduce and
// the chunk c - 1 results; fa_multi_select_layout picks the count by the model.
constexpr int kStripeChunks = 4;

// The arguments every round entry point checks, `who` naming it in the
// messages: the mode, the chunk count (0: the striped round's kStripeChunks,
// else 8; then 1..FA_COMM_MAX_CHUNKS), the exchange kind, root < nranks.
int check_round_args(const char* who, int mode, int* nchunks, int xchg, int root, int nranks);

// elem: FA_ELEM_F16 / FA_ELEM_BF16 builds the 16-bit table
// (fa_plan_build_host_elem), in 16-bit elements; another value is FA_E_INVAL.
int make_geo(int nranks, int rank, const int* counts, const fa_seg* seg32, int nseg32,
             int64_t f32_numel, const fa_seg* seg64, int nseg64, int64_t i64_numel,
             unsigned flags, const char* who, Geo* g, int elem = FA_ELEM_F32);

// What a 16-bit round supports: the striped form, unweighted (`who` names the
// entry in the message).  FA_ELEM_F32 passes everything.
int check_round_elem(const char* who, int elem, int mode, int weighted);
// ... with round options (fedagg_comm.h FA_ROUND_*): FA_ROUND_CHAIN16 admits
// the chained round, mean or weighted, on a 16-bit bucket and nothing else.
int check_round_opts(const char* who, int elem, int mode, int weighted, unsigned ropts);

// The cut of r->g for r->mode.  The tile lists are what a plan's device side
// is created from: chunk c = tiles [cut[c], cut[c + 1]) of g.t32 (e1, e2) or
// of `vec` (chained, blocked); `tails` / `tidx`: the compacted scalar fp32
// columns and their bucket indices.
int build_round(RoundGeo* r, int nchunks, std::vector<fa_tile_desc>* vec_out,
                std::vector<size_t>* cut_out, std::vector<fa_tile_desc>* tails_out,
                std::vector<int64_t>* tidx_out);

// The rank's operation list, as fa_describe_round returns it.
std::vector<fa_xfer> schedule(const RoundGeo& r, int root, bool weighted);

// ---------------------------------------------------------- stream rules ---
// One definition for the executor (fedcomm.hip execute) and the cost model.
inline bool is_comm(int op) { return op >= FA_X_SEND && op <= FA_X_BCAST; }
// (buffer, index) holds int64 elements: the stacked / gathered int64 keys
inline bool is_i64(int buf, int index) {
  return (buf == FA_B_STACK || buf == FA_B_GATHER) && index == 1;
}
// ... the ranks' fp32 weights (a weighted 16-bit chained round)
inline bool is_weights(int buf, int index) {
  return (buf == FA_B_STACK || buf == FA_B_GATHER) && index == 2;
}
bool on_comm_stream(const fa_xfer& x);
bool reads_exchanged(const fa_xfer& x);
bool user_written(int b);
bool needs_compute(const fa_xfer& x);

}  // namespace fa_sched
