// sched_host_check.cpp — runs the multi-GPU schedules and cost model
// (feddct_amd/csrc/sched_host.cpp) without HIP and without RCCL:
// g++ -std=c++17 sched_host_check.cpp sched_host.cpp plan_host.cpp, nothing
// else, no ROCm include path.
//
//   sched_host_check CASES OUT
//
// CASES (text, written by tests/golden/make_sched_host_golden.py case_file):
//   layout NAME F32_NUMEL I64_NUMEL N32 N64, then N32 + N64 lines "OFFSET NUMEL"
//   round NAME LAYOUT MODE NCHUNKS XCHG ROOT WEIGHTED W COUNT...
//   select NAME LAYOUT MFLAGS W COUNT...
// OUT: records [int32 len][name][int64 len][blob]:
//   NAME        of a round: per rank [int32 rc] and, accepted, [int32 nops] and
//               the raw fa_xfer array of fa_describe_round (56 B per op);
//   NAME/model  [int32 rc] and, accepted, the fa_round_cost bytes of fa_round_model;
//   NAME        of a selection: [int32 rc][int32 mode][int32 nchunks][double
//               model_us] of fa_multi_select_layout.
// Every accepted round is also checked here across its ranks, whatever the
// goldens say: steps never decrease; every send has a receive on the peer at
// the same position of that channel with the same count (and the reverse);
// every rank posts the same sequence of collectives; every offset + count
// lies inside the buffer it addresses.  Exit 0: every case ran and held.

#include <algorithm>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <tuple>
#include <vector>

#include "../../feddct_amd/csrc/sched_host.h"

static_assert(sizeof(fa_xfer) == 56, "fa_xfer is 56 B");
static_assert(sizeof(fa_round_cost) == 32, "fa_round_cost is 32 B");

int fa::set_err(int code, const char* fmt, ...) {
  (void)fmt;
  return code;
}

namespace {
using fa_sched::RoundGeo;

struct Segs {
  int64_t f32_numel = 0, i64_numel = 0;
  std::vector<fa_seg> s32, s64;
};

struct Blob {
  std::string b;
  void raw(const void* p, size_t n) { b.append((const char*)p, n); }
  void i32(int32_t v) { raw(&v, 4); }
};

[[noreturn]] void fail(const std::string& name, const std::string& why) {
  std::cerr << name << ": " << why << "\n";
  exit(1);
}

// [off, off + count) of (buf, index) lies inside the buffer as fedcomm.hip
// allocates and addresses it (make_round, addr) on the rank of geometry r.
// span: the elements the operation touches there.
void check_ref(const std::string& name, const RoundGeo& r, int buf, int index, int64_t off,
               int64_t span) {
  const fa_sched::Geo& g = r.g;
  auto in = [&](int64_t lo, int64_t hi, const char* what) {
    if (off < lo || span < 0 || off + span > hi) fail(name, std::string(what) + " range");
  };
  auto idx = [&](int n, const char* what) {
    if (index < 0 || index >= n) fail(name, std::string(what) + " index");
  };
  const bool striped = buf == FA_B_RECV || buf == FA_B_STRIPE;
  const bool owned = buf == FA_B_BLK || buf == FA_B_RELAY;
  if ((striped && r.lo.size() != (size_t)g.nranks + 1) ||
      (owned && r.bg.slo.size() != (size_t)g.nranks))
    fail(name, "a buffer of another round form");
  switch (buf) {
    case FA_B_NONE: return;
    case FA_B_CLIENT:
    case FA_B_WSTAGE:
      if (index != -1) idx(g.n_local, "client");
      return in(0, g.f32_numel, "client");
    case FA_B_OUT:
    case FA_B_PARTIAL:
    case FA_B_FIN: return in(0, g.f32_numel, "bucket");
    case FA_B_STATE:
      if (index != -1) idx(g.n_total >= 256 ? 4 : 2, "state plane");
      return in(0, g.f32_numel, "state plane");
    case FA_B_PIN:
    case FA_B_TAILP:
    case FA_B_CONT:
      if (index != -1) idx(4, "plane");
      return in(0, g.f32_numel, "plane");
    case FA_B_BSUM:
      if (index != -1) idx(r.bg.nbsum, "block sum");
      return in(0, g.f32_numel, "block sum");
    case FA_B_RECV:
      if (index != -1) idx(g.n_total, "receive row");
      return in(r.lo[g.rank], r.lo[g.rank + 1], "stripe");
    case FA_B_STRIPE: return in(r.lo[g.rank], r.lo[g.rank + 1], "stripe");
    case FA_B_BLK:
      if (index != -1) idx(std::max(1, r.bg.P), "piece");
      return in(r.bg.slo[g.rank], r.bg.shi[g.rank], "owner stripe");
    case FA_B_RELAY:
      idx(g.nranks, "relay row");
      return in(r.bg.slo[g.rank], r.bg.shi[g.rank], "owner stripe");
    case FA_B_STACK:
    case FA_B_GATHER: {
      if (index == -1) return in(0, 0, "stack");   // kernels name the whole stack
      idx(2, "stack");
      const int64_t rows = (int64_t)g.nmax * (buf == FA_B_GATHER ? g.nranks : 1);
      return in(0, rows * (index == 1 ? g.i64_numel : r.cg.t32_row), "stack");
    }
    default: fail(name, "unknown buffer");
  }
}

void check_round(const std::string& name, const std::vector<RoundGeo>& geo,
                 const std::vector<std::vector<fa_xfer>>& sch) {
  const int W = (int)sch.size();
  typedef std::tuple<int, int, int64_t, int64_t> Coll;   // op, root, offset, count
  std::vector<std::vector<Coll>> coll(W);
  std::map<std::pair<int, int>, std::vector<int64_t>> sends, recvs;   // (from, to) -> counts
  for (int r = 0; r < W; ++r) {
    int step = 0;
    for (const fa_xfer& x : sch[r]) {
      if (x.step < step) fail(name, "a step decreases");
      step = x.step;
      if (x.count < 0 || x.offset < 0) fail(name, "negative offset or count");
      if (x.op == FA_X_SEND || x.op == FA_X_RECV) {
        if (x.peer < 0 || x.peer >= W || x.peer == r) fail(name, "p2p peer");
        if (x.op == FA_X_SEND) sends[{r, x.peer}].push_back(x.count);
        else recvs[{x.peer, r}].push_back(x.count);
      } else if (fa_sched::is_comm(x.op)) {
        coll[r].emplace_back(x.op, x.peer, x.offset, x.count);
      } else if (x.nrows < 0 || x.row0 < 0 || x.row0 + x.nrows > geo[r].g.n_total) {
        fail(name, "kernel rows");
      }
      // an all-gather of per-rank rows fills W times its count
      const bool rows = x.op == FA_X_ALLGATHER && x.src != FA_B_PARTIAL;
      check_ref(name, geo[r], x.src, x.src_index, x.offset, x.count);
      check_ref(name, geo[r], x.dst, x.dst_index, x.offset, rows ? x.count * W : x.count);
    }
    if (coll[r] != coll[0]) fail(name, "ranks post different collectives");
  }
  if (sends != recvs) fail(name, "a channel's sends and receives do not match");
}

void run_round(const std::string& name, const Segs& L, int mode, int nchunks, int xchg, int root,
               int weighted, const std::vector<int>& counts,
               std::map<std::string, std::string>* out) {
  const int W = (int)counts.size();
  const unsigned flags = FA_PLAN_GAPS_ARE_PADDING;
  Blob b;
  std::vector<std::vector<fa_xfer>> sch(W);
  std::vector<RoundGeo> geo(W);
  bool all = true;
  for (int r = 0; r < W; ++r) {
    int n = 0;
    int rc = fa_describe_round(mode, W, r, counts.data(), L.s32.data(), (int)L.s32.size(),
                               L.f32_numel, L.s64.data(), (int)L.s64.size(), L.i64_numel, nchunks,
                               xchg, flags, root, weighted, nullptr, 0, &n);
    if (rc == FA_OK) {
      sch[r].resize(n);
      rc = fa_describe_round(mode, W, r, counts.data(), L.s32.data(), (int)L.s32.size(),
                             L.f32_numel, L.s64.data(), (int)L.s64.size(), L.i64_numel, nchunks,
                             xchg, flags, root, weighted, sch[r].data(), n, &n);
      if (rc != FA_OK || n != (int)sch[r].size()) fail(name, "the second call disagrees");
    }
    b.i32(rc);
    if (rc != FA_OK) {
      all = false;
      continue;
    }
    b.i32(n);
    b.raw(sch[r].data(), sch[r].size() * sizeof(fa_xfer));
    // the geometry the ops address, as fedcomm.hip make_round builds it
    RoundGeo& p = geo[r];
    p.mode = mode;
    p.xchg = xchg;
    int k = nchunks;
    if (fa_sched::check_round_args(name.c_str(), mode, &k, xchg, root, W)) fail(name, "arguments");
    p.req_chunks = k;
    std::vector<fa_tile_desc> vec, tails;
    std::vector<size_t> cut;
    std::vector<int64_t> tidx;
    if (fa_sched::make_geo(W, r, counts.data(), L.s32.data(), (int)L.s32.size(), L.f32_numel,
                           L.s64.data(), (int)L.s64.size(), L.i64_numel, flags, "check", &p.g) ||
        fa_sched::build_round(&p, k, &vec, &cut, &tails, &tidx))
      fail(name, "the geometry of an accepted round");
    if (fa_sched::schedule(p, root, weighted != 0).size() != sch[r].size())
      fail(name, "schedule() and fa_describe_round disagree");
  }
  if (all) check_round(name, geo, sch);
  (*out)[name] = b.b;
  Blob m;
  fa_round_cost c{};
  const int rc = fa_round_model(mode, W, counts.data(), L.s32.data(), (int)L.s32.size(),
                                L.f32_numel, L.s64.data(), (int)L.s64.size(), L.i64_numel, nchunks,
                                xchg, flags, root, weighted, &c);
  m.i32(rc);
  if (rc == FA_OK) m.raw(&c, sizeof c);
  (*out)[name + "/model"] = m.b;
}

void run_select(const std::string& name, const Segs& L, unsigned mflags,
                const std::vector<int>& counts, std::map<std::string, std::string>* out) {
  int mode = -1, nchunks = 0;
  double us = 0.0;
  const int rc = fa_multi_select_layout((int)counts.size(), counts.data(), L.s32.data(),
                                        (int)L.s32.size(), L.f32_numel, L.s64.data(),
                                        (int)L.s64.size(), L.i64_numel, FA_PLAN_GAPS_ARE_PADDING,
                                        mflags, &mode, &nchunks, &us);
  Blob b;
  b.i32(rc);
  b.i32(mode);
  b.i32(nchunks);
  b.raw(&us, 8);
  (*out)[name] = b.b;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::cerr << "usage: sched_host_check CASES OUT\n";
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
    int mode = 0, nchunks = 0, xchg = 0, root = 0, weighted = 0, W = 0;
    unsigned mflags = 0;
    if (cmd == "round") ss >> mode >> nchunks >> xchg >> root >> weighted;
    else if (cmd == "select") ss >> mflags;
    else fail(name, "unknown command " + cmd);
    ss >> W;
    std::vector<int> counts(std::max(0, W));
    for (int& c : counts) ss >> c;
    if (!ss || W < 1) fail(name, "bad case line");
    if (cmd == "round") run_round(name, layouts[lay], mode, nchunks, xchg, root, weighted, counts, &out);
    else run_select(name, layouts[lay], mflags, counts, &out);
    if (out.size() == before) fail(name, "a repeated case name");
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
