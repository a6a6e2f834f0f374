// plan_host_check.cpp — runs the host planners (feddct_amd/csrc/plan_host.cpp)
// without HIP: g++ -std=c++17 plan_host_check.cpp plan_host.cpp, nothing else.
//
//   plan_host_check CASES OUT
//
// CASES (text, written by tests/golden/make_plan_host_golden.py case_file):
//   layout NAME F32_NUMEL I64_NUMEL N32 N64, then N32 + N64 lines "OFFSET NUMEL"
//   default NAME LAYOUT TILE_ELEMS FLAGS ELEM S8 S16
//   tgpu NAME LAYOUT N FLAGS SLOTS_S1
// S8 / S16: the resident workgroups the 8- / 16-client kernels report.
// OUT: per case records [int32 len][name][int64 len][blob], the raw tables in
// the layout the golden generator dumps from the parent commit; a default
// case over fp32 elements is followed by NAME/launch, the launch rule's rows.
// Every table is also checked here, whatever the goldens say: its tiles are
// disjoint and cover exactly the segments' elements, a torch-GPU-order tile's
// stride bits are fa_torch_gpu_config's of its key, lo[] is monotone and
// ends at the tile count.  Exit 0: every case ran and held.

#include <algorithm>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../feddct_amd/csrc/plan_host.h"

int fa::set_err(int code, const char* fmt, ...) {
  (void)fmt;
  return code;
}

namespace {
using fa_host::Tile;
using namespace fa_k;

struct Segs {
  int64_t f32_numel = 0, i64_numel = 0;
  std::vector<fa_seg> s32, s64;
};

int g_s8 = 0, g_s16 = 0;
int slots_by_batch(int, int, int batch, bool, bool) { return batch == 16 ? g_s16 : g_s8; }

struct Blob {
  std::string b;
  void raw(const void* p, size_t n) { b.append((const char*)p, n); }
  void i32(int32_t v) { raw(&v, 4); }
  void i64(int64_t v) { raw(&v, 8); }
  template <class T>
  void vec(const std::vector<T>& v) { raw(v.data(), v.size() * sizeof(T)); }
};

const int kLaunchN[] = {1, 2, 7, 8, 11, 12, 16, 17, 63, 64, 128, 129, 200, 255, 256, 300};

[[noreturn]] void fail(const std::string& name, const std::string& why) {
  std::cerr << name << ": " << why << "\n";
  exit(1);
}

// Sorted, disjoint [start, end) pieces merged into maximal intervals; a piece
// that overlaps the one before it fails the case.
typedef std::vector<std::pair<int64_t, int64_t>> Spans;
Spans merged(const std::string& name, Spans s) {
  std::sort(s.begin(), s.end());
  Spans out;
  for (const auto& x : s) {
    if (!out.empty() && x.first < out.back().second) fail(name, "an element is covered twice");
    if (!out.empty() && x.first == out.back().second) out.back().second = x.second;
    else out.push_back(x);
  }
  return out;
}

// The elements of each bucket a table covers are exactly the segments'; with
// gaps_ok (FA_PLAN_GAPS_ARE_PADDING) a vector run may also cover fp32 gaps.
void check_cover(const std::string& name, const Segs& L, const std::vector<Tile>& tiles,
                 const std::vector<int64_t>* sidx, int64_t sidx_base, bool gaps_ok) {
  Spans got[2], want[2];
  for (const Tile& t : tiles) {
    if (t.count < 1) fail(name, "empty tile");
    if ((t.kind & 0xFF) == K_SCALAR_PACKED) {
      if (!sidx) fail(name, "packed tile without a scalar index");
      for (int i = 0; i < kPackCols; ++i) {
        const int64_t ent = (*sidx)[(size_t)(sidx_base + t.start + i)];
        if ((i < t.count) != (ent >= 0)) fail(name, "packed tile's entry count");
        if (ent >= 0) got[kind_is64((int)(ent & 15))].emplace_back(ent >> 4, (ent >> 4) + 1);
      }
      continue;
    }
    got[kind_is64(t.kind)].emplace_back(t.start, t.start + t.count);
  }
  for (int b = 0; b < 2; ++b) {
    for (const fa_seg& g : b ? L.s64 : L.s32)
      if (g.numel > 0) want[b].emplace_back(g.offset, g.offset + g.numel);
    const Spans g = merged(name, got[b]), w = merged(name, want[b]);
    if (!g.empty() && (g.front().first < 0 || g.back().second > (b ? L.i64_numel : L.f32_numel)))
      fail(name, "a tile outside its bucket");
    if (b == 0 && gaps_ok) {
      size_t i = 0;
      for (const auto& x : w) {
        while (i < g.size() && g[i].second <= x.first) ++i;
        if (i == g.size() || g[i].first > x.first || g[i].second < x.second)
          fail(name, "a segment's element is not covered");
      }
    } else if (g != w) {
      fail(name, "the tiles do not cover exactly the segments' elements");
    }
  }
}

void run_default(const std::string& name, const Segs& L, int tile_elems, unsigned flags, int elem,
                 std::map<std::string, std::string>* out) {
  // the host half of fedagg.hip plan_create_cpu
  fa_host::Layout l;
  int rc = fa_host::parse_layout("check", "", fa_host::kCheckSizes | fa_host::kCheckTile,
                                 L.s32.data(), (int)L.s32.size(), L.f32_numel, L.s64.data(),
                                 (int)L.s64.size(), L.i64_numel, tile_elems, flags, elem, &l);
  if (rc) fail(name, "parse_layout refused the case");
  const bool h16 = elem != FA_ELEM_F32, gaps = (flags & FA_PLAN_GAPS_ARE_PADDING) != 0;
  fa_host::PlanShape p;
  p.vec_u = l.info.tile_elems / (h16 ? fa_h16::kTile : 4 * kBlock);
  p.flags = h16 ? flags | FA_PLAN_TUNE_NO_BALANCE : flags;
  std::vector<Tile> tiles, alt;
  if (fa_host::build_tiles(l.s32, l.s64, l.info.tile_elems, flags, &tiles, &l.info, l.valign))
    fail(name, "build_tiles");
  if (l.autosel) {
    fa_plan_info ia{};
    if (fa_host::build_tiles(l.s32, l.s64, 4 * kBlock, flags, &alt, &ia)) fail(name, "alt table");
  }
  check_cover(name + " host", L, tiles, nullptr, 0, gaps);
  const fa_host::HostTables h =
      fa_host::plan_tables(tiles, alt, p.vec_u, p.flags, 0, slots_by_batch);
  p.nt = (int)h.main.size();
  p.ns = h.ns_main;
  p.nt_alt = (int)h.alt.size();
  p.ns_alt = h.ns_alt;
  check_cover(name + " main", L, h.main, &h.sidx, 0, gaps);
  if (!h.alt.empty()) check_cover(name + " alt", L, h.alt, &h.sidx, h.sidx_alt_off, gaps);
  Blob b;
  b.raw(&l.info, sizeof l.info);
  b.i32(fa_host::flat_bcast_ok(flags, l, elem, elem));
  b.i32(p.vec_u);
  b.i32(p.nt);
  b.i32(p.ns);
  b.i32(p.nt_alt);
  b.i32(p.ns_alt);
  b.i64(h.sidx_alt_off);
  b.i64((int64_t)h.sidx.size());
  b.vec(h.main);
  b.vec(h.alt);
  b.vec(h.sidx);
  b.i32((int32_t)h.bal.size());
  for (const fa_host::HostTables::Bal& t : h.bal) {
    check_cover(name + " balanced", L, t.tiles, &h.sidx, t.alt ? h.sidx_alt_off : 0, gaps);
    p.bal.push_back({t.u, t.slots, t.batch, (int)t.tiles.size(), t.alt});
    b.i32(t.u);
    b.i32(t.slots);
    b.i32(t.batch);
    b.i32(t.alt);
    b.i32((int32_t)t.tiles.size());
    b.vec(t.tiles);
  }
  (*out)[name] = b.b;
  if (h16) return;  // one table, launched as it is
  Blob r;
  for (int n : kLaunchN)
    for (int w = 0; w < 2; ++w) {
      const fa_host::Launch s = fa_host::select_launch(p, n, w != 0, slots_by_batch);
      for (int v : {s.table, s.nt, s.ns, s.vec_u, s.batch, s.slots, s.pipe}) r.i32(v);
    }
  (*out)[name + "/launch"] = r.b;
}

void run_tgpu(const std::string& name, const Segs& L, int n, unsigned flags, int slots,
              std::map<std::string, std::string>* out) {
  fa_host::Layout l;
  if (fa_host::parse_layout("check", "", 0, L.s32.data(), (int)L.s32.size(), L.f32_numel,
                            L.s64.data(), (int)L.s64.size(), L.i64_numel, 4 * kBlock, flags,
                            FA_ELEM_F32, &l))
    fail(name, "parse_layout refused the case");
  fa_host::TgpuTables t;
  const int rc = fa_host::plan_tgpu(l.s32, l.s64, n, flags, slots, &t);
  Blob b;
  b.i32(rc);
  if (rc == FA_OK) {
    check_cover(name, L, t.tiles, nullptr, 0, (flags & FA_PLAN_GAPS_ARE_PADDING) != 0);
    if (t.fac.size() != t.tiles.size()) fail(name, "one factor per tile");
    if (t.lo[0] != 0 || t.lo[5] != (int)t.tiles.size()) fail(name, "lo[] ends");
    for (int g = 0; g < 5; ++g)
      if (t.lo[g] > t.lo[g + 1]) fail(name, "lo[] not monotone");
    // a tile lies inside one key (or a run of keys of one stride): its stride
    // bits are the configuration of the key that holds its first element
    for (const Tile& x : t.tiles) {
      const fa_seg* key = nullptr;
      for (const fa_seg& g : kind_is64(x.kind) ? l.s64 : l.s32)
        if (g.numel > 0 && g.offset <= x.start && x.start < g.offset + g.numel) key = &g;
      int S = 0;
      if (!key || !fa_torch_gpu_config(n, key->numel, &S)) fail(name, "tile outside every key");
      if ((1 << ((x.kind >> 8) & 0xFF)) != S) fail(name, "tile's stride bits");
    }
    for (int g = 0; g < 6; ++g) b.i32(t.lo[g]);
    b.i32((int32_t)t.tiles.size());
    b.vec(t.tiles);
    b.vec(t.fac);
  }
  (*out)[name] = b.b;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::cerr << "usage: plan_host_check CASES OUT\n";
    return 2;
  }
  std::ifstream in(argv[1]);
  std::map<std::string, Segs> layouts;
  std::map<std::string, std::string> out;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string cmd, name, lay;
    if (!(ss >> cmd >> name)) continue;
    if (cmd == "layout") {
      Segs L;
      size_t n32 = 0, n64 = 0;
      ss >> L.f32_numel >> L.i64_numel >> n32 >> n64;
      for (size_t i = 0; i < n32 + n64; ++i) {
        fa_seg g{};
        if (!(in >> g.offset >> g.numel)) fail(name, "short layout");
        (i < n32 ? L.s32 : L.s64).push_back(g);
      }
      layouts[name] = L;
      continue;
    }
    ss >> lay;
    if (!layouts.count(lay)) fail(name, "unknown layout " + lay);
    const size_t before = out.size();
    if (cmd == "default") {
      int tile_elems = 0, elem = 0;
      unsigned flags = 0;
      ss >> tile_elems >> flags >> elem >> g_s8 >> g_s16;
      run_default(name, layouts[lay], tile_elems, flags, elem, &out);
    } else if (cmd == "tgpu") {
      int n = 0, slots = 0;
      unsigned flags = 0;
      ss >> n >> flags >> slots;
      run_tgpu(name, layouts[lay], n, flags, slots, &out);
    } else {
      fail(name, "unknown command " + cmd);
    }
    if (!ss || out.size() == before) fail(name, "bad case line");
  }
  std::ofstream o(argv[2], std::ios::binary);
  for (const auto& kv : out) {
    const int32_t nl = (int32_t)kv.first.size();
    const int64_t bl = (int64_t)kv.second.size();
    o.write((const char*)&nl, 4).write(kv.first.data(), nl);
    o.write((const char*)&bl, 8).write(kv.second.data(), bl);
  }
  return o.good() ? 0 : 1;
}
