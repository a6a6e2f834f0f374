// plan_host.cpp — the tile planners and launch rules (plan_host.h): segment
// checks, the default order's tile tables and their balanced re-cuts, the
// torch-GPU-order table, and the per-call choice of table and kernel form.
// Plain C++17: no HIP header, no HIP call.  Every rule below was tuned on a
// measurement, kept next to it.

#include "plan_host.h"

#include <algorithm>
#include <queue>
#include <utility>

namespace fa_host {
using fa::set_err;
using namespace fa_k;

namespace {
constexpr int kInline = FA_INLINE_CLIENTS;

inline int64_t body_len(int64_t M) {
  if (M >= 8) return (M / 32) * 32;
  if (M >= 2) return (M / 4) * 4;
  return 0;
}

int check_segs(const fa_seg* s, int ns, int64_t numel, const char* what,
               std::vector<fa_seg>* sorted) {
  if (ns < 0 || (ns > 0 && !s)) return set_err(FA_E_INVAL, "%s: bad segment array", what);
  sorted->assign(s, s + ns);
  std::stable_sort(sorted->begin(), sorted->end(),
                   [](const fa_seg& x, const fa_seg& y) { return x.offset < y.offset; });
  int64_t end = 0;
  for (const fa_seg& g : *sorted) {
    if (g.offset < 0 || g.numel < 0 || g.offset + g.numel > numel)
      return set_err(FA_E_INVAL, "%s: segment [%lld,+%lld) outside bucket of %lld", what,
                     (long long)g.offset, (long long)g.numel, (long long)numel);
    if (g.numel > 0 && g.offset < end)
      return set_err(FA_E_INVAL, "%s: overlapping segments at %lld", what, (long long)g.offset);
    if (g.numel > 0) end = g.offset + g.numel;
  }
  return FA_OK;
}

// May the broadcast copy the buckets flat?  Only when the caller declared the
// gaps padding (FA_PLAN_GAPS_ARE_PADDING) AND the segments, with that
// padding, cover the whole bucket: no gap (leading, between, trailing) of
// `pad` elements or more, i.e. no room for a key the plan does not own.  A
// plan over some of a layout's keys (a column chunk) keeps the tile-table
// broadcast, which writes its own tiles only.
bool covers_with_padding(const std::vector<fa_seg>& s, int64_t numel, int64_t pad) {
  int64_t pos = 0;
  for (const fa_seg& g : s) {
    if (g.numel == 0) continue;
    if (g.offset - pos >= pad) return false;
    pos = g.offset + g.numel;
  }
  return numel - pos < pad;
}

void push_scalar(std::vector<Tile>* t, int64_t start, int64_t count, int kind) {
  for (int64_t c = 0; c < count; c += kBlock)
    t->push_back(Tile{start + c, (int32_t)std::min<int64_t>(kBlock, count - c), kind});
}
}  // namespace

int check_flags(const char* who, unsigned flags, const char* hint) {
  if (flags & ~(unsigned)FA_PLAN_FLAGS_KNOWN)
    return set_err(FA_E_INVAL, "%s: unknown flag bits 0x%x%s", who,
                   flags & ~(unsigned)FA_PLAN_FLAGS_KNOWN, hint);
  return FA_OK;
}

int parse_layout(const char* who, const char* flags_hint, unsigned checks, const fa_seg* seg32,
                 int nseg32, int64_t f32_numel, const fa_seg* seg64, int nseg64,
                 int64_t i64_numel, int tile_elems, unsigned flags, int elem, Layout* out) {
  int rc = check_flags(who, flags, flags_hint);
  if (rc) return rc;
  if ((checks & kCheckSizes) && (f32_numel < 0 || i64_numel < 0))
    return set_err(FA_E_INVAL, "negative bucket size");
  const bool h16 = elem != FA_ELEM_F32;
  if (checks & kCheckTile) {
    if (elem != FA_ELEM_F32 && elem != FA_ELEM_F16 && elem != FA_ELEM_BF16)
      return set_err(FA_E_INVAL,
                     "%s: elem must be FA_ELEM_F32, FA_ELEM_F16 or FA_ELEM_BF16 (got %d)", who,
                     elem);
    out->autosel = !h16 && tile_elems == 0;
    if (h16) {
      // A 16-bit plan (FA_ELEM_F16 / FA_ELEM_BF16): the plain table of the
      // layout cut at 16-B vectors of 8 elements; its kernels
      // (fedagg_h16.hip) take one table at every client count.
      if (tile_elems == 0) tile_elems = fa_h16::kDefaultU * fa_h16::kTile;
      if (tile_elems != fa_h16::kTile && tile_elems != 2 * fa_h16::kTile)
        return set_err(FA_E_INVAL, "%s: a 16-bit plan's tile_elems must be 2048 or 4096 (got %d)",
                       who, tile_elems);
    } else {
      if (tile_elems == 0) tile_elems = 4 * kBlock * kDefaultU;
      if (tile_elems != 4 * kBlock && tile_elems != 8 * kBlock && tile_elems != 16 * kBlock)
        return set_err(FA_E_INVAL, "tile_elems must be 1024, 2048 or 4096 (got %d)", tile_elems);
    }
  }
  rc = check_segs(seg32, nseg32, f32_numel, h16 ? "16-bit" : "fp32", &out->s32);
  if (rc) return rc;
  rc = check_segs(seg64, nseg64, i64_numel, "int64", &out->s64);
  if (rc) return rc;
  out->valign = h16 ? fa_h16::kVec : 4;
  out->info = fa_plan_info{};
  out->info.f32_numel = f32_numel;
  out->info.i64_numel = i64_numel;
  out->info.tile_elems = tile_elems;
  return FA_OK;
}

// A 16-bit plan's broadcast copies the bucket's bytes flat, as numel / 2
// floats (a mixed plan's narrows element by element: any f32_numel); a gap
// of 128 16-bit elements is the 64-float gap of the fp32 rule.
bool flat_bcast_ok(unsigned flags, const Layout& l, int elem, int out_elem) {
  if (!(flags & FA_PLAN_GAPS_ARE_PADDING)) return false;
  const bool h16 = elem != FA_ELEM_F32;
  if (h16 && !(l.info.f32_numel % 2 == 0 || out_elem == FA_ELEM_F32)) return false;
  return covers_with_padding(l.s32, l.info.f32_numel, h16 ? 128 : 64) &&
         covers_with_padding(l.s64, l.info.i64_numel, 1);
}

// Every element belongs to at most one tile: two tiles over one element would
// race two summation orders (and two stores) into the same output.
int check_disjoint(std::vector<Tile> t, const char* who) {
  std::sort(t.begin(), t.end(), [](const Tile& x, const Tile& y) {
    const bool x64 = kind_is64(x.kind), y64 = kind_is64(y.kind);
    return x64 != y64 ? y64 : x.start < y.start;
  });
  for (size_t i = 1; i < t.size(); ++i)
    if (kind_is64(t[i - 1].kind) == kind_is64(t[i].kind) &&
        t[i - 1].start + t[i - 1].count > t[i].start)
      return set_err(FA_E_INVAL, "%s: tiles overlap at %s element %lld", who,
                     kind_is64(t[i].kind) ? "int64" : "fp32", (long long)t[i].start);
  return FA_OK;
}

// valign: elements per 16-B vector (4 fp32, 8 fp16 / bf16): a cascade body is
// vectorised when it starts and ends on that boundary.
int build_tiles(const std::vector<fa_seg>& s32, const std::vector<fa_seg>& s64, int tile_elems,
                unsigned flags, std::vector<Tile>* out, fa_plan_info* info, int valign) {
  std::vector<Tile> vec, tail;
  // Maximal runs of cascade-order elements, 16-B aligned (vectorisable).
  int64_t run_s = -1, run_e = -1;
  auto flush = [&]() {
    if (run_s < 0) return;
    for (int64_t c = run_s; c < run_e; c += tile_elems)
      vec.push_back(Tile{c, (int32_t)std::min<int64_t>(tile_elems, run_e - c), K_F32_VEC});
    info->cascade_elems += run_e - run_s;
    run_s = run_e = -1;
  };
  for (const fa_seg& g : s32) {
    const int64_t M = g.numel;
    if (M == 0) continue;
    if (M == 1) {
      // the scalar breaks the run: a later aligned segment must not extend
      // the open vector run across this element (it would be covered twice)
      flush();
      push_scalar(&tail, g.offset, 1, K_F32_INNER);
      info->tail_elems += 1;
      continue;
    }
    const int64_t b = body_len(M);
    if (b > 0) {
      if (g.offset % valign == 0 && b % valign == 0) {
        const bool extend = run_s >= 0 && (run_e == g.offset ||
                                           ((flags & FA_PLAN_GAPS_ARE_PADDING) && run_e <= g.offset));
        if (!extend) flush();
        if (run_s < 0) run_s = g.offset;
        run_e = g.offset + b;
      } else {
        flush();
        push_scalar(&tail, g.offset, b, K_F32_CASC_S);
        info->tail_elems += b;
      }
    }
    if (b < M) {
      flush();  // the tail breaks the run
      push_scalar(&tail, g.offset + b, M - b, K_F32_ILP4);
      info->tail_elems += M - b;
    }
  }
  flush();
  for (const fa_seg& g : s64) {
    const int64_t M = g.numel;
    if (M == 0) continue;
    if (M == 1) { push_scalar(&tail, g.offset, 1, K_I64_INNER); continue; }
    const int64_t b = body_len(M);
    if (b) push_scalar(&tail, g.offset, b, K_I64_CASC);
    if (b < M) push_scalar(&tail, g.offset + b, M - b, K_I64_ILP4);
  }
  std::vector<Tile> all(vec);
  all.insert(all.end(), tail.begin(), tail.end());
  const int rc = check_disjoint(all, "tile planner");
  if (rc) return rc;
  // Scalar tiles first: their few long-latency workgroups start early and
  // finish under the vector stream instead of trailing it.
  out->clear();
  out->insert(out->end(), tail.begin(), tail.end());
  out->insert(out->end(), vec.begin(), vec.end());
  info->ntiles = (int32_t)out->size();
  info->ntiles_cascade = (int32_t)vec.size();
  info->ntiles_tail = (int32_t)tail.size();
  return FA_OK;
}

// Clients per load batch of the reduce kernel a call runs (launch_reduce).
// r06: the 16-client kernels (three workgroups per CU) from 12 clients, with
// the client loop (pipe_rule): same process (profiles/r06_ab_lib_mid_n.jsonl)
// N = 12 / 14 / 16 -1.8 / -2.7 / -0.3 %, weighted N = 12 -1.4 / -1.5 % (C10 /
// C100); at N = 10 +1.0 %, so below 12 the 8-client kernels stay.
#ifndef FA_B16_MIN
#define FA_B16_MIN 12
#endif
int pick_batch(int n, int vec_u, unsigned pflags) {
  const int b = (pflags & FA_PLAN_TUNE_BATCH8)    ? 8
                : (pflags & FA_PLAN_TUNE_BATCH16) ? 16 : (n < FA_B16_MIN ? 8 : 16);
  return (vec_u == 4 && b == 16) ? 8 : b;  // no 16-client kernels at U = 4
}

// ------------------------------------------------------ balanced tables --
// One workgroup per tile: a launch of T equal tiles over `slots` resident
// workgroups (CUs x workgroups per CU) runs ceil(T / slots) rounds, and a
// part-filled round costs nearly a whole one while the launch is only one or
// two rounds long — measured r03 on one fp32 tensor of T x 2048 floats
// (tools/archive/exp_batch_cross.py, profiles/r03_exp_batch_cross*.jsonl), N = 20,
// 16-client kernel on 768 slots: 384 tiles 16.1 us, re-cut to 768 13.4 us;
// 768 tiles 22.7 us; 1,024 tiles 33.5 us, on the 8-client kernel's 1,280
// slots (one round) 28.3 us.  Past two rounds the tail is a small share and
// a re-cut (smaller, partial tiles) costs more than it saves: cfg4 weighted
// 144.2 vs 142.0 us, cfg5 185.5 vs 181.4 us, cfg3 43.7 vs 43.5 us re-cut vs
// plain (profiles/r03_exp_tune_balance.jsonl).  So a call of N >= 16
// clients whose plain table (a) part-fills ONE round of the 16-client kernel
// runs a table re-cut to fill it, (b) needs two rounds of the 16-client
// kernel but one of the 8-client kernel runs the 8-client kernel (resnet110sl
// sf4 N = 25, 923 tiles: 23.0 vs 26.3 us plain, 23.9 re-cut), (c) spills a
// few tiles past its last full round: the tail split below (split_tail), and
// (d) runs the plain table otherwise.  N < 16 (8-client kernel already) always runs
// plain: at N = 5 a re-cut is no gain (384 tiles 7.8 vs 9.0 us).
constexpr double kKeepFill = 0.97;  // the round at least this full: keep the plain table
constexpr int64_t kMinTile = 256;   // never cut vector tiles below this (elements)

// The slot count a plain (non-chain) reduce call runs on; 0 for a plan that
// launches its tiles as given (FA_PLAN_TUNE_NO_BALANCE).
int call_slots(int dev, int n, int vec_u, bool w, unsigned pflags, SlotFn slots) {
  if (pflags & FA_PLAN_TUNE_NO_BALANCE) return 0;
  return slots(dev, vec_u, pick_batch(n, vec_u, pflags), n >= 256, w);
}

namespace {
// Case (b) above: the batch a plain call of n clients runs with, given the
// plain table's tile count — 8 instead of 16 when that turns two rounds into
// one.  Explicit batch tuning flags and grid-shaping flags keep their batch.
int round_batch(int dev, int n, int vec_u, bool w, unsigned pflags, int ntiles, SlotFn slots) {
  const int b = pick_batch(n, vec_u, pflags);
  if (b != 16 || (pflags & (FA_PLAN_TUNE_BATCH16 | FA_PLAN_TUNE_NO_BALANCE))) return b;
  const int s16 = slots(dev, vec_u, 16, n >= 256, w);
  const int s8 = slots(dev, vec_u, 8, n >= 256, w);
  return (s16 > 0 && s8 > s16 && ntiles > s16 && ntiles <= s8) ? 8 : 16;
}

// A multi-round launch whose last round holds only r << slots tiles (r03
// session 4, tools/archive/exp_round_quant.py, profiles/r03_exp_round_quant.jsonl):
// those r tiles run alone, latency-bound, ~7-8 us after the last full round
// at N = 20 — cfg2's layout plus 16 / 18 / 25 extra 2048-float tiles (r = 1
// / 3 / 10 past 7 rounds of 768) reads 139.0 / 142.3 / 143.9 us against
// 136.3 us at 6.99 rounds, while 300 extra tiles cost only 146.4 us.  So the
// LAST slots - r vector tiles are split in halves (64-element lines): the
// table then fills exactly k rounds, its last round made of half tiles, and
// every earlier tile keeps the full width (re-cutting the whole table
// instead was slower, see above).  Same process, weighted, split vs plain
// (profiles/r03_exp_round_quant_tail_split*.jsonl): r = 10 137.9 vs 143.8
// us, r = 85 139.5 vs 144.0, r = 135 141.5 vs 144.8, r = 285 144.8 vs 146.3,
// r = 335 145.4 vs 147.6 — a gain at every r measured, up to 0.44 slots,
// so it is applied for 0 < r <= 0.44 slots (r03 applied it up to
// slots / 2, past the measured range).  A tile too small to halve (< 2 *
// kMinTile / 2 elements: ragged ends of runs) is left whole, so such a table
// may end up a few tiles short of exactly k rounds; the bits never change.
constexpr int64_t kTailMaxPct = 44;
std::vector<Tile> split_tail(const std::vector<Tile>& tiles, int64_t r, int slots) {
  if (r <= 0 || r * 100 > kTailMaxPct * (int64_t)slots) return {};
  std::vector<Tile> vec;
  for (const Tile& x : tiles)
    if (x.kind == K_F32_VEC) vec.push_back(x);
  const int64_t m = slots - r;  // tiles to split
  if ((int64_t)vec.size() < m) return {};
  std::vector<Tile> out;
  out.reserve(vec.size() + (size_t)m);
  const size_t first = vec.size() - (size_t)m;
  for (size_t i = 0; i < vec.size(); ++i) {
    const Tile& x = vec[i];
    const int64_t h = ((int64_t)x.count / 2) & ~(int64_t)63;
    if (i < first || h < kMinTile / 2) {
      out.push_back(x);
      continue;
    }
    out.push_back(Tile{x.start, (int32_t)h, K_F32_VEC});
    out.push_back(Tile{x.start + h, (int32_t)(x.count - h), K_F32_VEC});
  }
  return out;
}
}  // namespace

// The vector tiles of `tiles` (cut at cmax elements), re-cut for `slots`:
// only when they part-fill a single round (k = 1: slots - nscalar vector tiles),
// handed out run by run (a run = adjacent vector tiles) to the run whose
// tiles are largest, boundaries on 64-element (256 B) lines, no tile above
// cmax or (when split further) below kMinTile.  Empty: keep the plain table.
std::vector<Tile> balance_vec(const std::vector<Tile>& tiles, int cmax, int nscalar, int slots,
                              bool tail_only) {
  std::vector<std::pair<int64_t, int64_t>> runs;  // [start, end)
  int64_t t0 = 0;
  for (const Tile& x : tiles) {
    if (x.kind != K_F32_VEC) continue;
    ++t0;
    if (!runs.empty() && runs.back().second == x.start) runs.back().second += x.count;
    else runs.emplace_back(x.start, x.start + x.count);
  }
  if (t0 == 0 || slots <= 0) return {};
  const int64_t have = t0 + nscalar;
  const int64_t k = (have + slots - 1) / slots;
  if (k > 1) return split_tail(tiles, have - (k - 1) * slots, slots);
  if (tail_only || (double)have >= kKeepFill * (double)(k * slots)) return {};
  const int64_t target = k * slots - nscalar;
  std::vector<int64_t> m(runs.size());
  std::priority_queue<std::pair<double, size_t>> pq;  // (tile size, run), largest first
  int64_t total = 0;
  for (size_t r = 0; r < runs.size(); ++r) {
    const int64_t len = runs[r].second - runs[r].first;
    m[r] = (len + cmax - 1) / cmax;
    total += m[r];
    pq.emplace((double)len / (double)m[r], r);
  }
  while (total < target && !pq.empty()) {
    const size_t r = pq.top().second;
    pq.pop();
    const int64_t len = runs[r].second - runs[r].first;
    if ((double)len / (double)(m[r] + 1) < (double)kMinTile) break;  // every run is as small
    ++m[r];
    ++total;
    pq.emplace((double)len / (double)m[r], r);
  }
  if (total == t0) return {};
  std::vector<Tile> out;
  out.reserve((size_t)total + 16);
  for (size_t r = 0; r < runs.size(); ++r) {
    const int64_t s = runs[r].first, e = runs[r].second, len = e - s;
    for (int64_t mm = m[r];; ++mm) {
      const size_t mark = out.size();
      int64_t prev = s;
      bool ok = true;
      for (int64_t j = 1; j <= mm; ++j) {
        const int64_t b = j == mm ? e : ((s + j * len / mm) & ~(int64_t)63);
        if (b <= prev) continue;  // (a boundary rounded onto the previous one)
        if (b - prev > cmax) {
          ok = false;
          break;
        }
        out.push_back(Tile{prev, (int32_t)(b - prev), K_F32_VEC});
        prev = b;
      }
      if (ok) break;
      out.resize(mark);  // rounding pushed a tile past cmax: one more tile
    }
  }
  return out;
}

// The device form of a host tile table: its scalar tiles' columns, sorted by
// kind (a wave then mostly runs one order), packed kPackCols per K_SCALAR_PACKED
// tile with their entries appended to `sidx`; the vector tiles follow
// unchanged.  *nscalar = packed tiles (they lead the table, as the scalar
// tiles did).
std::vector<Tile> pack_scalar(const std::vector<Tile>& t, std::vector<int64_t>* sidx,
                              int* nscalar) {
  const int pack = kPackCols;
  std::vector<std::pair<int, int64_t>> cols;
  std::vector<Tile> vec;
  for (const Tile& x : t) {
    if (x.kind == K_F32_VEC) {
      vec.push_back(x);
      continue;
    }
    for (int32_t c = 0; c < x.count; ++c) cols.emplace_back(x.kind, x.start + c);
  }
  std::stable_sort(cols.begin(), cols.end(),
                   [](const std::pair<int, int64_t>& u, const std::pair<int, int64_t>& v) {
                     return u.first < v.first;
                   });
  std::vector<Tile> out;
  for (size_t c = 0; c < cols.size(); c += pack) {
    const int cnt = (int)std::min<size_t>(pack, cols.size() - c);
    out.push_back(Tile{(int64_t)sidx->size(), cnt, K_SCALAR_PACKED});
    for (int i = 0; i < kPackCols; ++i)
      sidx->push_back(i < cnt ? (cols[c + i].second << 4) | cols[c + i].first : -1);
  }
  *nscalar = (int)out.size();
  out.insert(out.end(), vec.begin(), vec.end());
  return out;
}

HostTables plan_tables(const std::vector<Tile>& tiles, const std::vector<Tile>& alt, int vec_u,
                       unsigned pflags, int dev, SlotFn slots) {
  HostTables h;
  h.main = pack_scalar(tiles, &h.sidx, &h.ns_main);
  if (!alt.empty()) {
    // the alt table's packed tiles index their own region of the scalar
    // index (the kernels get its base: tile k's entries at base + k * kPackCols)
    std::vector<int64_t> sa;
    h.alt = pack_scalar(alt, &sa, &h.ns_alt);
    h.sidx_alt_off = (int64_t)h.sidx.size();
    h.sidx.insert(h.sidx.end(), sa.begin(), sa.end());
  }
  // balanced tables for every slot count a call on this plan may run on
  // (main table: the 16-client kernels, deep or not, weighted or not; the
  // alt table: its unweighted 16-client kernels)
  if (pflags & FA_PLAN_TUNE_NO_BALANCE) return h;
  struct Req {
    int u, slots, batch;
    bool alt;
  };
  std::vector<Req> reqs;
  auto want = [&](int u, int s, int batch, bool a) {
    if (s <= 0) return;
    for (const Req& q : reqs)
      if (q.u == u && q.slots == s && q.batch == batch && q.alt == a) return;
    reqs.push_back(Req{u, s, batch, a});
  };
  // the 16-client kernels' calls: the whole rule; the calls of N < 16 (the
  // 8-client kernels): the tail split only (tools/archive/exp_tail_small_n.py: N = 5
  // / 8 / 12, 1.1-2.9 us per launch; a one-round re-cut is no gain there)
  for (int deep = 0; deep < 2; ++deep)
    for (int w = 0; w < 2; ++w) {
      if (pick_batch(16, vec_u, pflags) == 16)
        want(vec_u, slots(dev, vec_u, 16, deep != 0, w != 0), 16, false);
      const int b8 = pick_batch(8, vec_u, pflags);
      if (deep == 0) want(vec_u, slots(dev, vec_u, b8, false, w != 0), b8, false);
    }
  if (!h.alt.empty())
    for (int deep = 0; deep < 2; ++deep)
      want(1, slots(dev, 1, pick_batch(64, 1, pflags), deep != 0, false),
           pick_batch(64, 1, pflags), true);
  for (const Req& q : reqs) {
    const std::vector<Tile>& dev_t = q.alt ? h.alt : h.main;
    const int ns = q.alt ? h.ns_alt : h.ns_main;
    const std::vector<Tile> v =
        balance_vec(q.alt ? alt : tiles, q.u * 4 * kBlock, ns, q.slots, q.batch < 16);
    if (v.empty()) continue;
    HostTables::Bal b{q.u, q.slots, q.batch, q.alt, {}};
    b.tiles.assign(dev_t.begin(), dev_t.begin() + ns);  // the packed tiles lead
    b.tiles.insert(b.tiles.end(), v.begin(), v.end());
    h.bal.push_back(std::move(b));
  }
  return h;
}

// ---------------------------------------------- torch-ROCm's GPU order ----
extern "C" int fa_torch_gpu_config(int n, int64_t m, int* stride) {
  if (n < 2 || m < 1) return 0;
  auto last_pow2 = [](int64_t v) {
    int64_t p = 1;
    while (p * 2 <= v) p *= 2;
    return p;
  };
  auto div_up = [](int64_t a, int64_t b) { return (a + b - 1) / b; };
  int64_t S;
  if (m == 1) {
    // a 0-dim key stacked to [N]: lanes over the N values; from N >= 128 on
    // torch vectorises the input (tgpu_inner_vec), and N <= FA_MAX_CLIENTS
    // keeps values per thread below the cross-block threshold (N / 512 <
    // 256).  `stride` is the block width.
    S = n < 128 ? last_pow2(n) : std::min<int64_t>(last_pow2(n / 4), 512);
  } else {
    // setReduceConfig, "vectorize along output" ([N, M] reduced over dim 0,
    // iter.ndim() == 2), set_block_dimension with MAX_NUM_THREADS 512
    const int64_t ovs = m % 4 == 0 ? 4 : (m % 2 == 0 ? 2 : 1);
    const int64_t mnt = 512 / ovs, dim0 = m / ovs;
    const int64_t d0 = dim0 < mnt ? last_pow2(dim0) : mnt;
    const int64_t d1 = n < mnt ? last_pow2(n) : mnt;
    const int64_t bw0 = std::min<int64_t>(d0, 64);
    const int64_t bh = std::min<int64_t>(d1, mnt / bw0);
    const int64_t bw = std::min<int64_t>(d0, mnt / bh);
    const bool split = n >= std::min<int64_t>(bh * 16, 256);
    S = split ? bh : 1;
    if (S > 16) return 0;  // kernel limit (tgpu_kernel<LS>, LS <= 4)
    const int64_t vpt = div_up(n, S);
    if (split && vpt >= 256) {
      // the cross-block ("global") split: only when the output grid is
      // small against the target grid (kTorchNumCU CUs; max threads per CU
      // 256 for a 2-D iterator, the device's own for a single block —
      // ROCm's `uses_a_single_block` reads grid.x == 1)
      const int64_t grid = div_up(dim0, bw);
      const int64_t tpm = grid == 1 ? kTorchMaxThreadsPerCU : 256;
      const int64_t target = kTorchNumCU * (tpm / (bw * bh));
      if (grid <= target) {
        int64_t c = std::max(std::min(div_up(target, grid), div_up(vpt, 16)), div_up(vpt, 256));
        if (c > kTorchNumCU) c = kTorchNumCU;
        else if (c > div_up(kTorchNumCU, 2)) c = div_up(kTorchNumCU, 2);
        else if (c < 16) c = 1;
        if (c > 1) return 0;  // global_reduce: not restated
      }
    }
  }
  if (stride) *stride = (int)S;
  return 1;
}

// Rows per load batch of the S = 1 tiles for a plan cut for n clients: 8
// below 16 clients (as the default reduce's 8-client kernel; the 8-row form
// holds 102 VGPRs against 164, five workgroups per CU against three):
// measured r04 (tools/tgpu_speed.py, profiles/r04_tgpu_batch.jsonl) cfg3
// N = 5 40.8 vs 45.8 us, but cfg2 N = 20 146.7 vs 140.9, cfg5 N = 24 173.9
// vs 167.3.
// r06: from 10 clients the 16-row form (three workgroups per CU) since the
// client loop: same process (profiles/r06_ab_lib_tgpu_batch.jsonl) N = 10 / 12
// -1.7 / -2.5 %, N = 2 / 5 / sf32 (N = 3) +1.3 / +3.8 / +1.6 %.
#ifndef FA_TGPU_B16_MIN
#define FA_TGPU_B16_MIN 10
#endif
int tgpu_batch_for(int n) { return n < FA_TGPU_B16_MIN ? 8 : 16; }

namespace {
// The tail round of launch group gi (the S = 1 group, r04; the default
// plan's split_tail, §4.3 of DESIGN.md):
// its scalar and inner tiles first; and when its T tiles spill
// 0 < r <= 0.44 slots past k - 1 full rounds, the last slots - r wide tiles
// are halved (64-element lines), so the table fills exactly k rounds with a
// last round of half tiles instead of r tiles running alone.  cfg2 at N = 20: ~5,400 tiles on
// 768 slots = 7.03 rounds.  Per-column arithmetic: the bits never change.
void tgpu_split_tail(std::vector<Tile>* t, std::vector<float>* fac, int lo[6], int gi, int slots) {
  const int64_t T = lo[gi + 1] - lo[gi];
  const int64_t k = slots > 0 ? (T + slots - 1) / slots : 0;
  const int64_t r = T - (k - 1) * slots;
  // m: the wide tiles to halve (0: none; the group is still reordered so
  // its scalar and inner tiles — the int64 keys' one-wave latency chains —
  // run in the first round, as the default plan places its scalar tiles)
  const int64_t m = (k > 1 && r > 0 && r * 100 <= kTailMaxPct * (int64_t)slots) ? slots - r : 0;
  std::vector<Tile> nw, wd;
  std::vector<float> fnw, fwd;
  for (int64_t i = lo[gi]; i < lo[gi + 1]; ++i) {
    const bool w = ((*t)[i].kind & 0xFF) == K_F32_TGPU_W;
    (w ? wd : nw).push_back((*t)[i]);
    (w ? fwd : fnw).push_back((*fac)[i]);
  }
  std::vector<Tile> g(t->begin(), t->begin() + lo[gi]);
  std::vector<float> f(fac->begin(), fac->begin() + lo[gi]);
  g.insert(g.end(), nw.begin(), nw.end());
  f.insert(f.end(), fnw.begin(), fnw.end());
  const size_t first = (int64_t)wd.size() < m ? wd.size() : wd.size() - (size_t)m;
  for (size_t j = 0; j < wd.size(); ++j) {
    const Tile& x = wd[j];
    const int64_t h = ((int64_t)x.count / 2) & ~(int64_t)63;
    if (j < first || h < 64) {
      g.push_back(x);
      f.push_back(fwd[j]);
      continue;
    }
    g.push_back(Tile{x.start, (int32_t)h, x.kind});
    g.push_back(Tile{x.start + h, (int32_t)(x.count - h), x.kind});
    f.push_back(fwd[j]);
    f.push_back(fwd[j]);
  }
  const int add = (int)((int64_t)g.size() - lo[gi] - T);
  g.insert(g.end(), t->begin() + lo[gi + 1], t->end());
  f.insert(f.end(), fac->begin() + lo[gi + 1], fac->end());
  t->swap(g);
  fac->swap(f);
  for (int i = gi + 1; i < 6; ++i) lo[i] += add;
}
}  // namespace

int plan_tgpu(const std::vector<fa_seg>& s32, const std::vector<fa_seg>& s64, int n,
              unsigned flags, int slots_s1, TgpuTables* out) {
  return plan_tgpu(s32, s64, n, flags, slots_s1, out, 4);
}

// valign: elements per 16-B vector of the floating bucket.  4: the fp32 table
// above.  8 (fa_h16::kVec): a 16-bit bucket — vector tiles start and end on
// 8-element boundaries and hold up to fa_h16::kTile = 2048 elements at every
// row split (one 16-B load per lane per row); the (8 - offset % 8) % 8
// element head and the <= 7 element tail go to scalar tiles of the same S
// and factor.  Everything else — S and factor per key, runs across key
// boundaries, packed one-element keys, the grouping, the riders, lo[] — is
// the one rule.
int plan_tgpu(const std::vector<fa_seg>& s32, const std::vector<fa_seg>& s64, int n,
              unsigned flags, int slots_s1, TgpuTables* out, int valign) {
  if (valign != 4 && valign != fa_h16::kVec)
    return set_err(FA_E_INVAL, "torch-GPU order planner: vector alignment %d", valign);
  const bool h16 = valign == fa_h16::kVec;
  // elements of a wide (S <= 2) and of a vector (S >= 4) tile
  const int64_t te_w = h16 ? fa_h16::kTile : 8 * kBlock;
  const int64_t te_v = h16 ? fa_h16::kTile : 4 * kBlock;
  std::vector<Tile>& t = out->tiles;
  std::vector<float>& fac = out->fac;
  t.clear();
  fac.clear();
  // Wide S = 1 runs.  With S = 1 every M > 1 tensor has the same per-element
  // order (row p into accumulator p % 4, then ((a0 + a1) + a2) + a3), so the
  // 4-aligned bodies of adjacent such tensors with the same factor (bit for
  // bit) share one run cut into 2048-element tiles across key boundaries, as
  // the default plan's vector runs are: no partial tile per key (cfg2: 5432
  // -> ~5381 tiles).  Gaps join a run only when declared padding.
  // r06: runs of every row split S (the order depends on (N, S) only, as for
  // S = 1; S <= 2 in 2048-element W tiles, S >= 4 in 1024-element V tiles),
  // and adjacent one-element keys of one kind packed a wave each into one
  // tile: wrn16_8 C10 at N = 32 / 48 / 64 then fills 7 rounds of the S = 2
  // launch's 768 slots (5,372 tiles at each, 5,369 with the gaps declared
  // padding; pinned by tests/test_plan_host_cpu.py) where per-key tiles
  // spilled past them (5,417 / 5,417 / 5,432)
  int64_t run_s = -1, run_e = -1;
  int run_ls = 0;
  float run_f = 0.f;
  auto flush = [&]() {
    if (run_s < 0) return;
    const int64_t te = run_ls <= 1 ? te_w : te_v;
    const int kind = (run_ls <= 1 ? K_F32_TGPU_W : K_F32_TGPU_V) | (run_ls << 8);
    for (int64_t c = run_s; c < run_e; c += te) {
      t.push_back(Tile{c, (int32_t)std::min<int64_t>(te, run_e - c), kind});
      fac.push_back(run_f);
    }
    run_s = run_e = -1;
  };
  for (int pass = 0; pass < 2; ++pass) {
    flush();
    for (const fa_seg& g : pass ? s64 : s32) {
      if (g.numel == 0) continue;
      int S = 1;
      if (!fa_torch_gpu_config(n, g.numel, &S))
        return set_err(FA_E_RANGE,
                       "torch-GPU order: N=%d over a %lld-element tensor is outside the "
                       "restated configurations (cross-block split)", n, (long long)g.numel);
      int ls = 0;
      while ((1 << ls) < S) ++ls;
      // torch's factor: float(num_outputs) / numel, in float
      const float f = (float)g.numel / (float)((int64_t)n * g.numel);
      if (g.numel == 1) {
        flush();
        const int vec = n >= 128 ? 1 << 16 : 0;  // input-vectorised (tgpu_inner_vec)
        const int kind = (pass ? K_I64_TGPU_IN : K_F32_TGPU_IN) | (ls << 8) | vec;
        if (!t.empty() && t.back().kind == kind && fac.back() == f &&
            t.back().start + t.back().count == g.offset && t.back().count < kBlock / 64) {
          t.back().count++;   // one wave per element (tgpu_kernel's inner form)
          continue;
        }
        t.push_back(Tile{g.offset, 1, kind});
        fac.push_back(f);
        continue;
      }
      auto scalar = [&](int64_t lo, int64_t hi) {
        for (int64_t c = lo; c < hi; c += kBlock) {
          t.push_back(Tile{g.offset + c, (int32_t)std::min<int64_t>(kBlock, hi - c),
                           (pass ? K_I64_TGPU : K_F32_TGPU) | (ls << 8)});
          fac.push_back(f);
        }
      };
      if (pass) {
        scalar(0, g.numel);
        continue;
      }
      // fp32: the 16-B aligned body in 4-element-per-lane tiles, the <= 3
      // element head and tail one element per lane (same order, same factor)
      const int64_t head = std::min<int64_t>((valign - g.offset % valign) % valign, g.numel);
      const int64_t body = (g.numel - head) / valign * valign;
      // S = 1: 2048-element tiles, the default reduce's load shape (r02:
      // 151.9 us on cfg2 with the 1024-element form); S = 2 too since r05
      // (tgpu_wide_loop); a key whose body is not 16-B aligned keeps its own
      // tiles
      const bool wide = S <= 2;
      if (head == 0 && body > 0) {
        const bool extend = run_s >= 0 && run_f == f && run_ls == ls &&
                            (run_e == g.offset ||
                             ((flags & FA_PLAN_GAPS_ARE_PADDING) && run_e <= g.offset));
        if (!extend) flush();
        if (run_s < 0) {
          run_s = g.offset;
          run_f = f;
          run_ls = ls;
        }
        run_e = g.offset + body;
        if (body < g.numel) {
          flush();  // the tail breaks the run
          scalar(body, g.numel);
        }
        continue;
      }
      flush();
      scalar(0, head);
      const int64_t te = wide ? te_w : te_v;
      for (int64_t c = head; c < head + body; c += te) {
        t.push_back(Tile{g.offset + c, (int32_t)std::min<int64_t>(te, head + body - c),
                         (wide ? K_F32_TGPU_W : K_F32_TGPU_V) | (ls << 8)});
        fac.push_back(f);
      }
      scalar(head + body, g.numel);
    }
  }
  flush();
  const int rc = check_disjoint(t, "torch-GPU order planner");
  if (rc) return rc;
  // group the tiles by row split (inner tiles with S = 1): one launch each.
  // r05: when the S = 2 group holds the most tiles, the S = 1, S = 4 and
  // inner tiles ride in its launch, first (tgpu_kernel<1>; the small groups'
  // own launches cost 10-13 us of latency each at N = 32..127).  With the
  // S = 2 tiles wide, same process against the build before
  // (profiles/r05_ab_lib_tgpu_s2.jsonl): N = 32 / 48 / 64 / 100 / 127
  // -10.0 / -10.2 / -12.2 / -10.6 / -7.8 %, C100 N = 64 / 128 -11.6 / -6.0 %
  // (0.83-0.85 of 8 TB/s); S = 1 riders only: 1-3 points less
  std::vector<int> grp(t.size());
  int cnt[5] = {0, 0, 0, 0, 0};
  for (size_t i = 0; i < t.size(); ++i) {
    const int b = t[i].kind & 0xFF;
    grp[i] = (b == K_F32_TGPU_IN || b == K_I64_TGPU_IN) ? 0 : (t[i].kind >> 8) & 0xFF;
    cnt[grp[i]]++;
  }
  const bool ride = cnt[1] > 0 && cnt[1] >= cnt[0] && cnt[1] >= cnt[2];
  // sort key: launch group, riders before the group's own tiles
  std::vector<int> key(t.size());
  for (size_t i = 0; i < t.size(); ++i) {
    const bool rider = ride && (grp[i] == 0 || grp[i] == 2);
    // tgpu_kernel<1> reduces every vector (V) rider with the S = 4 path: S = 1
    // keys never make V tiles (wide = S <= 2 above); refuse a table that
    // would, rather than reduce it in the wrong order
    if (rider && (t[i].kind & 0xFF) == K_F32_TGPU_V && ((t[i].kind >> 8) & 0xFF) != 2)
      return set_err(FA_E_INVAL, "torch-GPU order planner: a vector rider of row split %d",
                     1 << ((t[i].kind >> 8) & 0xFF));
    if (rider) grp[i] = 1;
    key[i] = 2 * grp[i] + (rider ? 0 : 1);
  }
  std::vector<size_t> ord(t.size());
  for (size_t i = 0; i < ord.size(); ++i) ord[i] = i;
  std::stable_sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return key[x] < key[y]; });
  std::vector<Tile> t2;
  std::vector<float> f2;
  for (size_t i : ord) {
    t2.push_back(t[i]);
    f2.push_back(fac[i]);
  }
  t.swap(t2);
  fac.swap(f2);
  int* lo = out->lo;
  for (int g = 0; g < 6; ++g) lo[g] = 0;
  for (size_t i = 0; i < ord.size(); ++i) lo[grp[ord[i]] + 1]++;
  for (int g = 0; g < 5; ++g) lo[g + 1] += lo[g];
  // r06: the same halving on the S = 2 launch measured neutral at
  // N = 32 / 64 / 100, -2.7 % at N = 48, +0.5 % on C100 N = 128
  // (profiles/r06_ab_lib_tgpu_runs.jsonl, variant "nobal"): not applied
  if (!(flags & FA_PLAN_TUNE_NO_BALANCE)) tgpu_split_tail(&t, &fac, lo, 0, slots_s1);
  return FA_OK;
}

int plan_order_elem(const char* who, const fa_seg* seg32, int nseg32, int64_t f32_numel,
                    const fa_seg* seg64, int nseg64, int64_t i64_numel, int n, int order,
                    unsigned flags, int elem, int slots_s1, Layout* l, TgpuTables* out) {
  int rc = check_flags(who, flags);
  if (rc) return rc;
  if (order != FA_ORDER_TORCH_GPU) return set_err(FA_E_INVAL, "%s: order %d", who, order);
  if (n < 2 || n > FA_MAX_CLIENTS)
    return set_err(FA_E_RANGE, "%s: n=%d outside 2..%d", who, n, FA_MAX_CLIENTS);
  // (tile_elems 0: the element type's own width; a 16-bit table is cut in
  // fa_h16::kTile-element tiles whatever it says)
  rc = parse_layout(who, "", kCheckSizes | kCheckTile, seg32, nseg32, f32_numel, seg64, nseg64,
                    i64_numel, 0, flags, elem, l);
  if (rc) return rc;
  return plan_tgpu(l->s32, l->s64, n, flags, (flags & FA_PLAN_TUNE_NO_BALANCE) ? 0 : slots_s1,
                   out, l->valign);
}

// -------------------------------------------------------- launch rules --
namespace {
// The next client's loads before the current client's adds
// (reduce_impl.h pipe2_clients) where it measured faster
// (profiles/r05_exp_pipe2_*.jsonl, r05_ab_lib_pipe2_*.jsonl): calls of 2..7
// or 17..63 clients (inline pointers), mean or weighted, on the full
// 2048-float tiles of launches of three or more rounds of resident
// workgroups (partial tiles — tensor ends, the halved tail of a table re-cut
// for the round count — keep the batch form).  Not the 1024-float table, not
// 8..16 clients (r05: on the 8-client kernels), not the short launches
// (resnet110sl N = 25 at two rounds: +0.9 %; sf32 N = 3 at 2.5: +0.8 %).
// r06: 12..16 clients on the 16-client kernels (pick_batch, FA_B16_MIN);
// unweighted calls of 64..128 clients too, now on the 2048-float table
// (select_launch): same process against the 1024-float table's batch form
// (profiles/r06_ab_lib_n64.jsonl, two boxes) C10 N = 64 / 100 / 128 -3.5 /
// -3.1 / -3.2 % and -3.1 / -2.5 / -2.6 %, C100 N = 64 / 100 -3.0 / -2.5 % and
// -0.3 / -2.2 %, bits equal; the 2048-float table in the batch form alone
// -1.8 / -3.0 / -3.3 / -1.8 / -2.0 %.  Weighted calls from 64 keep the batch
// form (r05: the loop +0.4 / +2.4 % at 80 / 128; r06 again: -0.7 / +0.3 /
// +1.2 / +3.2 % at 64 / 80 / 100 / 128, profiles/r06_ab_lib_w64_loop.jsonl).
int pipe_rule(const Launch& L, int n, bool weighted) {
  // r06: unweighted calls of 256 clients and more (the DEEP cascade) on the
  // 2048-float table, the loop reading the device pointer table through
  // scalar loads (PIPE = 2): same process against the 1024-float table's
  // batch form (profiles/r06_ab_lib_tab_loop.jsonl) N = 256 / 300 -1.9 /
  // -3.8 %; at 129..255 (not deep) +0.2 / +3.5 % at 150 / 200, so those keep
  // the 1024-float table.  Bits equal.
  if (n > kInline)
    return (!weighted && n >= 256 && L.vec_u == 2 && L.batch == 16 && L.slots > 0 &&
            L.nt >= 3 * L.slots)
               ? 2
               : 0;
  if (L.vec_u != 2 || L.slots <= 0 || L.nt < 3 * L.slots) return 0;
#ifndef FA_PIPE_MID_LO
#define FA_PIPE_MID_LO FA_B16_MIN
#endif
  return (n >= 2 && n <= 7) || (n >= FA_PIPE_MID_LO && n <= 63) || (!weighted && n >= 64) ? 1
                                                                                            : 0;
}
}  // namespace

Launch select_launch(const PlanShape& plan, int n, bool weighted, SlotFn slots) {
  Launch L{kTableMain, false, plan.nt, plan.ns, plan.vec_u, 0, 0, 0};
  // 1024-float tiles for unweighted calls of 129..255 clients (r02's
  // tools/tune.py sweep took them from N = 64; r06: 64..128 and from 256 run
  // faster on the 2048-float table with the client loop, see pipe_rule; the
  // 2048-float table at N = 200 +3.7 % in the batch form, +3.5 % with the loop)
  if (plan.nt_alt > 0 && !weighted && n > kInline && n < 256) {
    L.table = kTableAlt;
    L.alt = true;
    L.nt = plan.nt_alt;
    L.ns = plan.ns_alt;
    L.vec_u = 1;
  }
  // the batch: 8 where that runs the plain table in one round instead of two
  L.batch = round_batch(plan.device, n, L.vec_u, weighted, plan.flags, L.nt, slots);
  L.slots = call_slots(plan.device, n, L.vec_u, weighted, plan.flags, slots);
  if (L.batch != pick_batch(n, L.vec_u, plan.flags)) {
    L.slots = slots(plan.device, L.vec_u, L.batch, n >= 256, weighted);
  } else {
    // the table cut for the slot count of the kernel this call runs
    for (size_t i = 0; i < plan.bal.size(); ++i) {
      const PlanShape::Bal& b = plan.bal[i];
      if (b.slots == L.slots && b.u == L.vec_u && b.alt == L.alt && b.batch == L.batch) {
        L.table = (int)i;
        L.nt = b.nt;
        break;
      }
    }
  }
  L.pipe = pipe_rule(L, n, weighted);
  return L;
}

}  // namespace fa_host

// ---- host-only C ABI (fedagg.h); sched_host.cpp calls the first and last --
using fa::set_err;
using namespace fa_k;

namespace {
// One body behind fa_plan_build_host and fa_plan_build_host_elem.
int plan_build_host(const char* who, const fa_seg* seg32, int nseg32, int64_t f32_numel,
                    const fa_seg* seg64, int nseg64, int64_t i64_numel, int tile_elems,
                    unsigned flags, int elem, fa_tile_desc* tiles, int cap, fa_plan_info* info) {
  if (!info) return set_err(FA_E_INVAL, "%s: info is NULL", who);
  fa_host::Layout l;
  int rc = fa_host::parse_layout(who, "", fa_host::kCheckTile, seg32, nseg32, f32_numel, seg64,
                                 nseg64, i64_numel, tile_elems, flags, elem, &l);
  if (rc) return rc;
  std::vector<Tile> t;
  rc = fa_host::build_tiles(l.s32, l.s64, l.info.tile_elems, flags, &t, &l.info, l.valign);
  if (rc) return rc;
  *info = l.info;
  if (tiles) {
    if (cap < (int)t.size())
      return set_err(FA_E_RANGE, "%s: %d tiles, capacity %d", who, (int)t.size(), cap);
    for (size_t i = 0; i < t.size(); ++i) tiles[i] = fa_tile_desc{t[i].start, t[i].count, t[i].kind};
  }
  return FA_OK;
}
}  // namespace

extern "C" {

int fa_plan_build_host(const fa_seg* seg32, int nseg32, int64_t f32_numel, const fa_seg* seg64,
                       int nseg64, int64_t i64_numel, int tile_elems, unsigned flags,
                       fa_tile_desc* tiles, int cap, fa_plan_info* info) {
  return plan_build_host("fa_plan_build_host", seg32, nseg32, f32_numel, seg64, nseg64, i64_numel,
                         tile_elems, flags, FA_ELEM_F32, tiles, cap, info);
}

int fa_plan_build_host_elem(const fa_seg* seg32, int nseg32, int64_t f32_numel,
                            const fa_seg* seg64, int nseg64, int64_t i64_numel, int tile_elems,
                            unsigned flags, int elem, fa_tile_desc* tiles, int cap,
                            fa_plan_info* info) {
  if (elem == FA_ELEM_F32)
    return fa_plan_build_host(seg32, nseg32, f32_numel, seg64, nseg64, i64_numel, tile_elems,
                              flags, tiles, cap, info);
  return plan_build_host("fa_plan_build_host_elem", seg32, nseg32, f32_numel, seg64, nseg64,
                         i64_numel, tile_elems, flags, elem, tiles, cap, info);
}

int fa_plan_build_order_host_elem(const fa_seg* seg32, int nseg32, int64_t f32_numel,
                                  const fa_seg* seg64, int nseg64, int64_t i64_numel, int n,
                                  int order, unsigned flags, int elem, int slots,
                                  fa_tile_desc* tiles, float* factors, int cap, int* lo,
                                  int* ntiles) {
  const char* who = "fa_plan_build_order_host_elem";
  if (!ntiles) return set_err(FA_E_INVAL, "%s: ntiles is NULL", who);
  if (slots < 0 || cap < 0) return set_err(FA_E_INVAL, "%s: bad arguments", who);
  fa_host::Layout l;
  fa_host::TgpuTables t;
  const int rc = fa_host::plan_order_elem(who, seg32, nseg32, f32_numel, seg64, nseg64, i64_numel,
                                          n, order, flags, elem, slots, &l, &t);
  if (rc) return rc;
  *ntiles = (int)t.tiles.size();
  if (lo)
    for (int g = 0; g < 6; ++g) lo[g] = t.lo[g];
  if (tiles || factors) {
    if (cap < (int)t.tiles.size())
      return set_err(FA_E_RANGE, "%s: %d tiles, capacity %d", who, (int)t.tiles.size(), cap);
    for (size_t i = 0; i < t.tiles.size(); ++i) {
      if (tiles) tiles[i] = fa_tile_desc{t.tiles[i].start, t.tiles[i].count, t.tiles[i].kind};
      if (factors) factors[i] = t.fac[i];
    }
  }
  return FA_OK;
}

int fa_plan_balance_host(const fa_tile_desc* vec, int nvec, int tile_elems, int nscalar,
                         int slots, fa_tile_desc* out, int cap) {
  if (nvec < 0 || (nvec > 0 && !vec) || nscalar < 0 || slots < 0 || cap < 0 ||
      (cap > 0 && !out))
    return set_err(FA_E_INVAL, "fa_plan_balance_host: bad arguments");
  if (tile_elems != 4 * kBlock && tile_elems != 8 * kBlock && tile_elems != 16 * kBlock)
    return set_err(FA_E_INVAL, "tile_elems must be 1024, 2048 or 4096 (got %d)", tile_elems);
  std::vector<Tile> t;
  for (int i = 0; i < nvec; ++i) {
    if (vec[i].kind != K_F32_VEC || vec[i].count < 4 || vec[i].count % 4 ||
        vec[i].count > tile_elems || vec[i].start % 4)
      return set_err(FA_E_INVAL, "fa_plan_balance_host: tile %d is not a vector tile", i);
    t.push_back(Tile{vec[i].start, vec[i].count, vec[i].kind});
  }
  const std::vector<Tile> b = fa_host::balance_vec(t, tile_elems, nscalar, slots);
  if ((int64_t)b.size() > (int64_t)cap)
    return set_err(FA_E_RANGE, "fa_plan_balance_host: %zu tiles > cap %d", b.size(), cap);
  for (size_t i = 0; i < b.size(); ++i) out[i] = fa_tile_desc{b[i].start, b[i].count, b[i].kind};
  return (int)b.size();
}

unsigned fa_chain_levels(int rows, int n_total) {
  if (rows <= 0 || n_total < 1) return 0;
  const int lp = level_power(n_total);
  const int step = 1 << lp;
  unsigned m = 0;
  if (rows % step) m |= 1u;                     // the open block
  if ((rows >> lp) % step) m |= 2u;             // completed blocks since the last promotion
  if (n_total >= 256) {                         // levels 2-3 exist (DEEP kernels)
    if ((rows >> (2 * lp)) % step) m |= 4u;
    if (rows >> (3 * lp)) m |= 8u;              // level 3 only accumulates
  }
  return m;
}

}  // extern "C"
