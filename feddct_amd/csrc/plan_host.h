// plan_host.h — the tile planners and launch rules of libfedagg.so: host
// arithmetic over segment lists and tile counts, no HIP (plan_host.cpp is
// compiled as plain C++ and runs without a device).  Whatever a rule needs
// to know of the device reaches it as a number: the resident-workgroup
// counts of the kernels, through SlotFn.  fedagg.hip owns the occupancy
// queries, the uploads, the C ABI and the launches.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/fedagg.h"
#include "err.h"
#include "tiles.h"

namespace fa_host {
using fa_k::Tile;

// Resident workgroups of the reduce kernel (U, batch, deep, weighted) on
// device `dev` (0: unknown -> the plain table); fedagg.hip kernel_slots.
typedef int (*SlotFn)(int dev, int u, int batch, bool deep, bool weighted);

// ------------------------------------------------------------- layouts --
int check_flags(const char* who, unsigned flags, const char* hint = "");

// A plan entry point's layout arguments, checked: the segment lists sorted
// by offset, the tile width resolved, `info`'s sizes and tile width filled.
struct Layout {
  std::vector<fa_seg> s32, s64;
  fa_plan_info info{};
  int valign = 4;        // elements per 16-B vector of the floating bucket
  bool autosel = false;  // fp32 with tile_elems == 0: the plan also carries the 1024-float table
};
enum : unsigned {
  kCheckSizes = 1u,  // the bucket sizes are not negative (the create paths)
  kCheckTile = 2u,   // elem is known and tile_elems one of its widths (0: its default)
};
// The checks of every plan entry point, in the order they have always been
// made: flag bits, bucket sizes, element type and tile width, the floating
// segments, the int64 segments.  `who` names the entry point in the
// messages; the floating bucket is called "fp32" or "16-bit" after `elem`.
int parse_layout(const char* who, const char* flags_hint, unsigned checks, const fa_seg* seg32,
                 int nseg32, int64_t f32_numel, const fa_seg* seg64, int nseg64,
                 int64_t i64_numel, int tile_elems, unsigned flags, int elem, Layout* out);

bool flat_bcast_ok(unsigned flags, const Layout& l, int elem, int out_elem);
int check_disjoint(std::vector<Tile> t, const char* who);
int build_tiles(const std::vector<fa_seg>& s32, const std::vector<fa_seg>& s64, int tile_elems,
                unsigned flags, std::vector<Tile>* out, fa_plan_info* info, int valign = 4);

// ------------------------------------------------------- table cutting --
std::vector<Tile> balance_vec(const std::vector<Tile>& tiles, int cmax, int nscalar, int slots,
                              bool tail_only = false);
std::vector<Tile> pack_scalar(const std::vector<Tile>& t, std::vector<int64_t>* sidx,
                              int* nscalar);

// A default-order plan's device tables, on the host: the main and the alt
// (1024-float, may be empty) table with their scalar tiles packed, the
// scalar index both share (the alt table's region from sidx_alt_off), and
// the balanced tables for every slot count a call on the plan may run on.
struct HostTables {
  std::vector<Tile> main, alt;
  int ns_main = 0, ns_alt = 0;  // leading packed tiles
  std::vector<int64_t> sidx;
  int64_t sidx_alt_off = 0;
  struct Bal {
    int u, slots;
    int batch;  // clients per load batch of the kernel it was cut for
    bool alt;   // cut from the alt table: its scalar index region
    std::vector<Tile> tiles;
  };
  std::vector<Bal> bal;
};
HostTables plan_tables(const std::vector<Tile>& tiles, const std::vector<Tile>& alt, int vec_u,
                       unsigned pflags, int dev, SlotFn slots);

// --------------------------------------------------- torch-GPU order ----
int tgpu_batch_for(int n);
// The torch-GPU-order table of a layout for n clients: tiles, their mean
// factors, and the launch groups lo[g]..lo[g+1] by row split S = 1..16.
// slots_s1: resident workgroups of the S = 1 group's kernel (0: unknown).
struct TgpuTables {
  std::vector<Tile> tiles;
  std::vector<float> fac;
  int lo[6] = {0, 0, 0, 0, 0, 0};
};
int plan_tgpu(const std::vector<fa_seg>& s32, const std::vector<fa_seg>& s64, int n,
              unsigned flags, int slots_s1, TgpuTables* out);
// The same for a floating bucket of `valign` elements per 16-B vector: 4 is
// the table above; 8 cuts a 16-bit bucket's (fa_plan_create_order_elem).
int plan_tgpu(const std::vector<fa_seg>& s32, const std::vector<fa_seg>& s64, int n,
              unsigned flags, int slots_s1, TgpuTables* out, int valign);
// One body behind fa_plan_create_order_elem's 16-bit arm and
// fa_plan_build_order_host_elem: the argument checks of the two parents
// (flags, order, n, elem, segments) in their order and the table of a
// torch-GPU-order plan over a bucket of `elem` elements.
int plan_order_elem(const char* who, const fa_seg* seg32, int nseg32, int64_t f32_numel,
                    const fa_seg* seg64, int nseg64, int64_t i64_numel, int n, int order,
                    unsigned flags, int elem, int slots_s1, Layout* l, TgpuTables* out);

// -------------------------------------------------------- launch rules --
// What a launch decision reads of a default-order plan.
struct PlanShape {
  int device = 0;
  unsigned flags = 0;
  int vec_u = fa_k::kDefaultU;
  int nt = 0, ns = 0;          // the main device table: tiles, leading packed tiles
  int nt_alt = 0, ns_alt = 0;  // the alt table (nt_alt == 0: none)
  struct Bal {
    int u, slots, batch, nt;
    bool alt;
  };
  std::vector<Bal> bal;
};
// The table and kernel form a plain reduce call runs with.
enum : int { kTableMain = -1, kTableAlt = -2 };  // >= 0: index into PlanShape::bal
struct Launch {
  int table;
  bool alt;  // the alt table's scalar index region, 1024-float tiles
  int nt, ns;
  int vec_u;
  int batch;  // clients per load batch of its kernel
  int slots;  // resident workgroups of its kernel (0: unknown / tuning grid)
  int pipe;   // 0: the batch form; 1 / 2: the client loop (reduce_impl.h pipe2_clients)
};
int pick_batch(int n, int vec_u, unsigned pflags);
int call_slots(int dev, int n, int vec_u, bool w, unsigned pflags, SlotFn slots);
Launch select_launch(const PlanShape& plan, int n, bool weighted, SlotFn slots);

}  // namespace fa_host
