// tgpu16_host_check.cpp — the torch-GPU-order planner for 16-bit buckets
// (feddct_amd/csrc/plan_host.cpp, fa_plan_build_order_host_elem) from plain
// C++, without HIP and without Python:
//
//   g++ -std=c++17 [-fsanitize=address,undefined] -o tgpu16_host_check
//       tgpu16_host_check.cpp ../../feddct_amd/csrc/plan_host.cpp
//   ./tgpu16_host_check
//
// Layouts: one key per size of kSizes plus an int64 0-dim key, and a raw
// segment list whose keys start at every residue mod 8, back to back and
// across gaps; both 16-bit element types, with and without
// FA_PLAN_GAPS_ARE_PADDING, N in kNs, three slot counts.  Every table is
// checked here: each segment element in exactly one tile, no tile over a gap
// that is not padding, vector tiles on 8-element boundaries and at most 2048
// elements, each tile's row split fa_torch_gpu_config's and its factor
// float(M) / float(N M) of its key, lo[] monotone and grouped by S.  With
// FA_ELEM_F32 the entry must return plan_tgpu's table.  The refusals hold.
// Exit 0 and "N cases held" when everything did.

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../feddct_amd/csrc/plan_host.h"

static char g_msg[512];
int fa::set_err(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof g_msg, fmt, ap);
  va_end(ap);
  return code;
}

namespace {
using namespace fa_k;

const int64_t kSizes[] = {1, 2, 3, 6, 8, 16, 36, 100, 128, 2047, 2048, 4097, 3 * 2048,
                          5 * 2048 + 100};
const int kNs[] = {2, 9, 17, 32, 64, 128, 256};
const int kSlots[] = {0, 8, 768};

struct Lay {
  std::vector<fa_seg> s32, s64;
  int64_t n32 = 0, n64 = 0;
};

[[noreturn]] void fail(const std::string& what, const char* why) {
  fprintf(stderr, "%s: %s (last error: %s)\n", what.c_str(), why, g_msg);
  exit(1);
}

Lay key_layout(int n) {
  Lay l;
  int64_t off = 0;
  for (int64_t m : kSizes) {
    if (!fa_torch_gpu_config(n, m, nullptr)) continue;  // outside the restatement at this N
    l.s32.push_back(fa_seg{off, m});
    off = (off + m + 7) / 8 * 8;
  }
  l.n32 = off + 64;
  l.s64.push_back(fa_seg{0, 1});
  l.n64 = 1;
  return l;
}

// (the small key: 9 elements, 33 from N = 256 on, where every key below 32
// elements is outside the restatement)
Lay raw_layout(int n) {
  Lay l;
  int64_t off = 0;
  const int64_t small = n < 256 ? 9 : 33;
  for (int r = 0; r < 8; ++r) {
    off = (off + 7) / 8 * 8 + r;
    for (int64_t m : {(int64_t)2048 + 17, small, (int64_t)1, (int64_t)40 + r}) {
      l.s32.push_back(fa_seg{off, m});
      off += m;
    }
    off += 3;
  }
  off = (off + 7) / 8 * 8;
  for (int64_t m : {128, 256, 4096}) {
    l.s32.push_back(fa_seg{off, m});
    off += m;
  }
  off += 16;
  l.s32.push_back(fa_seg{off, 512});
  off += 512;
  l.s32.push_back(fa_seg{off, 1});
  off += 8;
  l.s32.push_back(fa_seg{off, 64});
  off += 64;
  l.n32 = (off + 7) / 8 * 8 + 64;
  l.s64.push_back(fa_seg{0, 1});
  l.s64.push_back(fa_seg{3, 36});
  l.n64 = 40;
  return l;
}

struct Table {
  std::vector<fa_tile_desc> t;
  std::vector<float> f;
  int lo[6];
};

int build(const Lay& l, int n, unsigned flags, int elem, int slots, Table* out) {
  int nt = -1;
  int rc = fa_plan_build_order_host_elem(l.s32.data(), (int)l.s32.size(), l.n32, l.s64.data(),
                                         (int)l.s64.size(), l.n64, n, FA_ORDER_TORCH_GPU, flags,
                                         elem, slots, nullptr, nullptr, 0, nullptr, &nt);
  if (rc) return rc;
  out->t.assign((size_t)nt, fa_tile_desc{});
  out->f.assign((size_t)nt, 0.f);
  // (capacity exactly the count: a write past it is the sanitizer's to find)
  return fa_plan_build_order_host_elem(l.s32.data(), (int)l.s32.size(), l.n32, l.s64.data(),
                                       (int)l.s64.size(), l.n64, n, FA_ORDER_TORCH_GPU, flags,
                                       elem, slots, out->t.data(), out->f.data(), nt, out->lo,
                                       &nt);
}

void check(const std::string& name, const Lay& l, int n, unsigned flags, int elem,
           const Table& tb) {
  const bool h16 = elem != FA_ELEM_F32;
  const int vec = h16 ? 8 : 4;
  std::vector<int> key32((size_t)l.n32, -1), key64((size_t)l.n64, -1);
  std::vector<int> cov32((size_t)l.n32, 0), cov64((size_t)l.n64, 0);
  for (size_t i = 0; i < l.s32.size(); ++i)
    for (int64_t e = 0; e < l.s32[i].numel; ++e) key32[(size_t)(l.s32[i].offset + e)] = (int)i;
  for (size_t i = 0; i < l.s64.size(); ++i)
    for (int64_t e = 0; e < l.s64[i].numel; ++e) key64[(size_t)(l.s64[i].offset + e)] = (int)i;
  if (tb.lo[0] != 0 || tb.lo[5] != (int)tb.t.size()) fail(name, "lo[] does not span the table");
  for (int g = 0; g < 5; ++g)
    if (tb.lo[g] > tb.lo[g + 1]) fail(name, "lo[] not monotone");
  for (size_t i = 0; i < tb.t.size(); ++i) {
    const fa_tile_desc& t = tb.t[i];
    const int base = t.kind & 0xFF, ls = (t.kind >> 8) & 0xFF, vbit = (t.kind >> 16) & 1;
    const bool is64 = kind_is64(t.kind);
    const bool inner = base == K_F32_TGPU_IN || base == K_I64_TGPU_IN;
    const bool vtile = base == K_F32_TGPU_V || base == K_F32_TGPU_W;
    if (!(vtile || inner || base == K_F32_TGPU || base == K_I64_TGPU)) fail(name, "tile kind");
    const int64_t lim = is64 ? l.n64 : l.n32;
    if (t.count <= 0 || t.start < 0 || t.start + t.count > lim) fail(name, "tile outside bucket");
    if (vtile) {
      if (t.start % vec || t.count % vec) fail(name, "vector tile off a 16-B boundary");
      const int cap = h16 ? 2048 : (base == K_F32_TGPU_W ? 2048 : 1024);
      if (t.count > cap) fail(name, "vector tile too large");
      if ((ls <= 1) != (base == K_F32_TGPU_W)) fail(name, "wide / vector tile kind vs row split");
    } else if (t.count > (inner ? kBlock / 64 : kBlock)) {
      fail(name, "scalar tile too large");
    }
    bool any = false;
    for (int64_t e = t.start; e < t.start + t.count; ++e) {
      ++(is64 ? cov64 : cov32)[(size_t)e];
      const int k = (is64 ? key64 : key32)[(size_t)e];
      if (k < 0) continue;
      any = true;
      const int64_t m = (is64 ? l.s64 : l.s32)[(size_t)k].numel;
      int S = 0;
      if (!fa_torch_gpu_config(n, m, &S) || S != (1 << ls)) fail(name, "row split");
      if (inner != (m == 1) || vbit != (inner && n >= 128 ? 1 : 0)) fail(name, "inner form");
      const float f = (float)m / (float)((int64_t)n * m);
      if (memcmp(&f, &tb.f[i], 4) != 0) fail(name, "factor");
    }
    if (!any) fail(name, "a tile over no key");
    int g = 0;
    while (!(tb.lo[g] <= (int)i && (int)i < tb.lo[g + 1])) ++g;
    const int own = inner ? 0 : ls;
    if (!(g == own || (g == 1 && (own == 0 || own == 2)))) fail(name, "launch group");
  }
  for (int64_t e = 0; e < l.n32; ++e) {
    const int c = cov32[(size_t)e];
    if (key32[(size_t)e] >= 0 ? c != 1 : (flags & FA_PLAN_GAPS_ARE_PADDING) ? c > 1 : c != 0)
      fail(name, "16-bit / fp32 coverage");
  }
  for (int64_t e = 0; e < l.n64; ++e)
    if (cov64[(size_t)e] != (key64[(size_t)e] >= 0 ? 1 : 0)) fail(name, "int64 coverage");
}

void same_as_plan_tgpu(const std::string& name, const Lay& l, int n, unsigned flags, int slots) {
  Table tb;
  if (build(l, n, flags, FA_ELEM_F32, slots, &tb)) fail(name, "the fp32 table was refused");
  fa_host::TgpuTables ref;
  if (fa_host::plan_tgpu(l.s32, l.s64, n, flags, slots, &ref)) fail(name, "plan_tgpu refused");
  if (ref.tiles.size() != tb.t.size()) fail(name, "fp32 table: tile count");
  for (size_t i = 0; i < tb.t.size(); ++i)
    if (ref.tiles[i].start != tb.t[i].start || ref.tiles[i].count != tb.t[i].count ||
        ref.tiles[i].kind != tb.t[i].kind || memcmp(&ref.fac[i], &tb.f[i], 4) != 0)
      fail(name, "fp32 table differs from plan_tgpu's");
  if (memcmp(ref.lo, tb.lo, sizeof ref.lo) != 0) fail(name, "fp32 table: lo[]");
}

int refusal(const Lay& l, int n, int order, unsigned flags, int elem) {
  int nt = 0;
  return fa_plan_build_order_host_elem(l.s32.data(), (int)l.s32.size(), l.n32, nullptr, 0, 0, n,
                                       order, flags, elem, 0, nullptr, nullptr, 0, nullptr, &nt);
}
}  // namespace

int main() {
  int cases = 0;
  for (int n : kNs) {
    const Lay keys = key_layout(n), raw = raw_layout(n);
    for (unsigned flags : {0u, (unsigned)FA_PLAN_GAPS_ARE_PADDING})
      for (int slots : kSlots) {
        for (int elem : {FA_ELEM_F16, FA_ELEM_BF16, FA_ELEM_F32})
          for (int which = 0; which < 2; ++which) {
            const Lay& l = which ? raw : keys;
            const std::string name = std::string(which ? "raw" : "keys") + "/n" +
                                     std::to_string(n) + "/f" + std::to_string(flags) + "/s" +
                                     std::to_string(slots) + "/e" + std::to_string(elem);
            Table tb;
            if (build(l, n, flags, elem, slots, &tb)) fail(name, "refused");
            check(name, l, n, flags, elem, tb);
            ++cases;
          }
        same_as_plan_tgpu("keys/f32/n" + std::to_string(n), keys, n, flags, slots);
        same_as_plan_tgpu("raw/f32/n" + std::to_string(n), raw, n, flags, slots);
        cases += 2;
      }
  }
  // the two element types cut the same table (the kind carries no type)
  const Lay raw = raw_layout(32);
  {
    Table a, b;
    if (build(raw, 32, 1, FA_ELEM_F16, 768, &a) || build(raw, 32, 1, FA_ELEM_BF16, 768, &b))
      fail("same", "refused");
    if (a.t.size() != b.t.size() ||
        memcmp(a.t.data(), b.t.data(), a.t.size() * sizeof(fa_tile_desc)) != 0)
      fail("same", "fp16 and bf16 tables differ");
    ++cases;
  }
  // refusals
  Lay one;
  one.s32.push_back(fa_seg{0, 1024});
  one.n32 = 1024;
  const int G = FA_ORDER_TORCH_GPU;
  if (refusal(one, 2, G, 0, FA_ELEM_BF16) != FA_OK) fail("refusals", "N = 2 refused");
  if (refusal(one, 1, G, 0, FA_ELEM_BF16) != FA_E_RANGE) fail("refusals", "N = 1");
  if (refusal(one, 0, G, 0, FA_ELEM_F16) != FA_E_RANGE) fail("refusals", "N = 0");
  if (refusal(one, FA_MAX_CLIENTS + 1, G, 0, FA_ELEM_F16) != FA_E_RANGE) fail("refusals", "N max");
  if (refusal(one, 4, G, 0, 7) != FA_E_INVAL) fail("refusals", "unknown elem");
  if (refusal(one, 4, G, 0x40u, FA_ELEM_BF16) != FA_E_INVAL) fail("refusals", "unknown flag bits");
  if (refusal(one, 4, FA_ORDER_TORCH_CPU, 0, FA_ELEM_BF16) != FA_E_INVAL) fail("refusals", "order");
  if (refusal(one, 512, G, 0, FA_ELEM_BF16) != FA_E_RANGE ||
      !strstr(g_msg, "outside the restated configurations"))
    fail("refusals", "(N = 512, M = 1024) is a cross-block key");
  if (refusal(one, 512, G, 0, FA_ELEM_F32) != FA_E_RANGE) fail("refusals", "cross-block, fp32");
  {
    Lay bad = one;
    bad.s32.push_back(fa_seg{512, 8});
    if (refusal(bad, 4, G, 0, FA_ELEM_BF16) != FA_E_INVAL) fail("refusals", "overlap");
    bad = one;
    bad.n32 = 1000;
    if (refusal(bad, 4, G, 0, FA_ELEM_BF16) != FA_E_INVAL) fail("refusals", "outside bucket");
    fa_tile_desc small[1];
    int nt = 0;
    if (fa_plan_build_order_host_elem(raw.s32.data(), (int)raw.s32.size(), raw.n32, nullptr, 0, 0,
                                      4, G, 0, FA_ELEM_BF16, 0, small, nullptr, 1, nullptr,
                                      &nt) != FA_E_RANGE || nt <= 1)
      fail("refusals", "capacity");
  }
  cases += 12;
  printf("%d cases held\n", cases);
  return 0;
}
