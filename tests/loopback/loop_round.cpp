// loop_round.cpp — TEST DRIVER: the native multi-rank rounds of
// libfedagg_comm (chained, striped, sharded with either e1 exchange) run with
// W ranks on one GPU over the loopback communicator (loopccl.hip), for one or
// several rounds on ONE plan per rank, every round checked against one GPU's
// fa_reduce over all clients:
//   chained / striped / blocked / multi / mean_multi: bit-identical (fp32 and
//   int64; mean_multi has no int64 keys; two NaNs are equal whatever their
//   payload, tests/helpers.bits_equal's convention);
//   sharded / multi_e1 (e1): int64 bit-identical, fp32 within the forward
//   error bound of two N-term sums, 2N * 2^-24 * sum_i |w_i x_i| (any
//   summation order), from that round's data and weights.
// Usage: loop_round LAYOUT CASE...
//   LAYOUT: "f32_numel i64_numel nseg32 nseg64 [P]" then one "offset numel"
//           line per segment (fp32 first), as BucketLayout.segs32 / segs64;
//           with P, fp32 lines are "offset numel key mu sigma" and int64
//           lines "offset numel key": the digest generator's per-key
//           parameters (feddct_amd/workload.py fill_client), so a result can
//           be checked against tests/golden/digests.json (FA_LOOP_DUMP).
//   CASE:   mode:W:counts:root:model:weighted:nchunks[:script]
//           mode   chained | striped | blocked | sharded | sharded_rs
//                  | multi (the default entry: fa_multi_plan_create /
//                    fa_reduce_multi) | multi_e1 (FA_MULTI_REASSOCIATE)
//                  | mean_multi (fa_mean_f32_multi: fp32 keys only)
//           counts comma-separated client slots per rank (sum = N)
//           root   result rank, or -1 for every rank
//           model  threads (one thread + comm per rank: fa_comm_init_rank)
//                  | single (one thread drives all ranks: fa_comm_init; only
//                    for schedules whose p2p pairs share a step: sharded, blocked)
//           script comma list, one entry per round: the round's root and m
//                  (mean) or w (weighted), e.g. 0m,-1w,2w,0m; the entry `a`
//                  is no round: it makes the data adversarial (fa_synth_fill_*
//                  mode 1: exponents 2^-20..2^20, random signs).  With round
//                  entries the case's own root and weighted fields are not
//                  used; without any (no script, or `a` alone) the case is
//                  one round of them.
// A script runs on one plan and one communicator per rank.  Round k fills
// client slot i with the generator's client i + k * n and weighs it with
// ((i + 3k) mod n + 1) / sum; every round's reference is computed before the
// ranks start.  Each rank NaN-fills its result buckets on its stream, runs the
// round, copies the result to the round's slot and refills its own client
// buckets IN PLACE with the next round's data on its stream — the round's
// last act joined that stream to the communication stream, so this is the
// supported use — with no host synchronisation between rounds.  Everything is
// compared after one final synchronisation; the client buckets then still
// hold the last round's data, bit for bit (a round never writes its inputs).
// One JSON line per case; exit status 0 iff every case passed.  rounds: the
// script's length; bad_round: the first failing round (from 1; 0: none) and
// bad_first / bad_last its bad fp32 elements; round_ok: per round;
// bad_inputs: client words a round changed.
// FA_LOOP_CLIENTS=path: round 0's fp32 client buckets, raw float32
// [n][f32_numel], instead of the generator's (special values);
// FA_LOOP_WEIGHTS=path: round 0's n float32 weights.
// FA_LOOP_DUMP=path: the first result rank's out32 then out64, raw, of the
// last case's last round.
// FA_LOOP_GATE_MS=ms (threads model, scripts): after every round but the last,
// each rank queues a one-thread spin kernel of that length on its stream
// BEFORE it refills its client buckets for the next round, and issues the next
// round at once: every launch of that round is queued while its inputs still
// hold the previous round's data, so work that the executor puts on its
// communication stream without joining the caller's stream reads stale values
// and the round's result is wrong.  A round whose call returns after its gate
// has ended fails the case ("gate too short / call blocked the host").
// FA_LOOP_PROFILE=1 (threads model): every rank's communicator profiles its
// rounds (fa_comm_set_profile) and the line carries rank 0's
// fa_round_plan_profile of the last.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "fedagg.h"
#include "fedagg_comm.h"

namespace {

struct Layout {
  int64_t f32_numel = 0, i64_numel = 0;
  std::vector<fa_seg> s32, s64;
  bool params = false;                 // per-key generator parameters given
  std::vector<int> key32, key64;
  std::vector<float> mu, sigma;
};

struct Round {
  int root = -1, weighted = 0;
};

struct Case {
  std::string mode, model, text;
  int W = 0, root = -1, weighted = 0, nchunks = 0;
  std::vector<int> counts;
  std::vector<Round> rounds;  // one entry per round on the plan
  int data_mode = 0;          // fa_synth_fill_* mode: 0 realistic, 1 adversarial
};

bool read_layout(const char* path, Layout* L) {
  FILE* f = fopen(path, "r");
  if (!f) return false;
  char line[256];
  long long a, b;
  int n32, n64;
  char tag[8] = {0};
  if (!fgets(line, sizeof line, f)) return false;
  const int got = sscanf(line, "%lld %lld %d %d %7s", &a, &b, &n32, &n64, tag);
  if (got < 4) return false;
  L->params = got == 5 && tag[0] == 'P';
  L->f32_numel = a;
  L->i64_numel = b;
  for (int i = 0; i < n32 + n64; ++i) {
    long long o, m;
    if (fscanf(f, "%lld %lld", &o, &m) != 2) return false;
    (i < n32 ? L->s32 : L->s64).push_back(fa_seg{o, m});
    if (!L->params) continue;
    int k;
    if (fscanf(f, "%d", &k) != 1) return false;
    if (i < n32) {
      float mu, sg;
      if (fscanf(f, "%f %f", &mu, &sg) != 2) return false;
      L->key32.push_back(k);
      L->mu.push_back(mu);
      L->sigma.push_back(sg);
    } else {
      L->key64.push_back(k);
    }
  }
  fclose(f);
  return true;
}

bool parse_case(const std::string& s, Case* c) {
  std::vector<std::string> f;
  std::stringstream ss(s);
  std::string tok;
  while (std::getline(ss, tok, ':')) f.push_back(tok);
  if (f.size() != 7 && f.size() != 8) return false;
  c->text = s;
  c->mode = f[0];
  c->W = atoi(f[1].c_str());
  std::stringstream cs(f[2]);
  while (std::getline(cs, tok, ',')) c->counts.push_back(atoi(tok.c_str()));
  c->root = atoi(f[3].c_str());
  c->model = f[4];
  c->weighted = atoi(f[5].c_str());
  c->nchunks = atoi(f[6].c_str());
  if (f.size() == 8) {
    std::stringstream rs(f[7]);
    while (std::getline(rs, tok, ',')) {
      if (tok == "a") {
        c->data_mode = 1;
        continue;
      }
      // <root><m|w>
      if (tok.size() < 2) return false;
      const char kind = tok.back();
      if (kind != 'm' && kind != 'w') return false;
      char* end = nullptr;
      const std::string num = tok.substr(0, tok.size() - 1);
      const long root = strtol(num.c_str(), &end, 10);
      if (!end || *end || root < -1 || root >= c->W) return false;
      c->rounds.push_back(Round{(int)root, kind == 'w'});
    }
  }
  if (c->rounds.empty()) c->rounds.push_back(Round{c->root, c->weighted});
  return (int)c->counts.size() == c->W;
}

#define HIPC(x)                                                             \
  do {                                                                      \
    if ((x) != hipSuccess) {                                                \
      fprintf(stderr, "%s failed\n", #x);                                   \
      exit(2);                                                              \
    }                                                                       \
  } while (0)

// FA_LOOP_GATE_MS: one thread spins until `ticks` of the constant-rate wall
// clock have passed.  `cap` bounds the trips as well (a trip is a clock read:
// tens of nanoseconds at least, so 2^20 trips per millisecond asked for is far
// beyond the gate and still well under a second per 10 ms), so the kernel ends
// whatever the clock or its reported rate do.
__global__ void gate_kernel(long long ticks, long long cap) {
  const long long t0 = wall_clock64();
  for (long long i = 0; i < cap && wall_clock64() - t0 < ticks; ++i) {
  }
}

// Words of a[0..n) that differ from b's (the inputs' check: bit for bit).
__global__ void count_diff_kernel(const uint32_t* a, const uint32_t* b, int64_t n,
                                  unsigned long long* bad) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    if (a[i] != b[i]) atomicAdd(bad, 1ull);
}

void count_diff(const void* a, const void* b, int64_t words, unsigned long long* bad) {
  if (words <= 0) return;
  const unsigned grid = (unsigned)std::min<int64_t>(1024, (words + 255) / 256);
  hipLaunchKernelGGL(count_diff_kernel, dim3(grid), dim3(256), 0, nullptr, (const uint32_t*)a,
                     (const uint32_t*)b, words, bad);
  HIPC(hipGetLastError());
}

struct Rank {
  fa_comm* comm = nullptr;
  void* plan = nullptr;
  hipStream_t st = nullptr;
  std::vector<float*> c32;      // this rank's client buckets (refilled in place)
  std::vector<int64_t*> c64;
  int slot0 = 0;                // its first slot
  float* out32 = nullptr;       // result buckets (a result rank of any round)
  int64_t* out64 = nullptr;
  float* save32 = nullptr;      // [rounds][F]: each round's result
  int64_t* save64 = nullptr;    // [rounds][I]
  hipEvent_t gate_end = nullptr;  // FA_LOOP_GATE_MS: the end of the last gate on st
  bool gated = false;
  int rc = 0;
  std::string err;
  fa_round_profile prof{};
  bool has_prof = false;
};

int create_plan(const Case& c, const Layout& L, Rank& r) {
  const unsigned fl = FA_PLAN_GAPS_ARE_PADDING;
  const fa_seg* s64 = L.s64.empty() ? nullptr : L.s64.data();
  if (c.mode == "mean_multi") return 0;  // stateless: cached in the communicator
  if (c.mode == "multi" || c.mode == "multi_e1")
    return fa_multi_plan_create(r.comm, L.s32.data(), (int)L.s32.size(), L.f32_numel, s64,
                                (int)L.s64.size(), L.i64_numel, c.counts.data(), c.nchunks, fl,
                                c.mode == "multi" ? FA_MULTI_EXACT : FA_MULTI_REASSOCIATE,
                                (fa_multi_plan**)&r.plan);
  if (c.mode == "chained")
    return fa_chain_plan_create(r.comm, L.s32.data(), (int)L.s32.size(), L.f32_numel, s64,
                                (int)L.s64.size(), L.i64_numel, c.counts.data(), c.nchunks, fl,
                                (fa_chain_plan**)&r.plan);
  if (c.mode == "striped")
    return fa_stripe_plan_create_ex(r.comm, L.s32.data(), (int)L.s32.size(), L.f32_numel, s64,
                                    (int)L.s64.size(), L.i64_numel, c.counts.data(), c.nchunks,
                                    fl, (fa_stripe_plan**)&r.plan);
  if (c.mode == "blocked")
    return fa_block_plan_create(r.comm, L.s32.data(), (int)L.s32.size(), L.f32_numel, s64,
                                (int)L.s64.size(), L.i64_numel, c.counts.data(), fl,
                                (fa_block_plan**)&r.plan);
  return fa_shard_plan_create_ex(r.comm, L.s32.data(), (int)L.s32.size(), L.f32_numel, s64,
                                 (int)L.s64.size(), L.i64_numel, c.counts.data(), c.nchunks,
                                 c.mode == "sharded_rs" ? FA_XCHG_RS_GATHER : FA_XCHG_REDUCE, fl,
                                 (fa_shard_plan**)&r.plan);
}

int run_round(const Case& c, const Layout& L, int root, std::vector<Rank*>& ranks,
              std::vector<void*>& plans, std::vector<fa_shard_io>& io) {
  const int nl = (int)plans.size();
  if (c.mode == "mean_multi") {
    if (nl != 1) return -1;  // one thread per rank only
    return fa_mean_f32_multi(ranks[0]->comm, io[0].c32, c.counts.data(), L.f32_numel,
                             io[0].out32, L.s32.data(), (int)L.s32.size(), root, io[0].stream);
  }
  if (c.mode == "multi" || c.mode == "multi_e1")
    return fa_reduce_multi((fa_multi_plan* const*)plans.data(), nl, io.data(), root);
  if (c.mode == "chained")
    return fa_reduce_chained((fa_chain_plan* const*)plans.data(), nl, io.data(), root);
  if (c.mode == "striped")
    return fa_reduce_striped((fa_stripe_plan* const*)plans.data(), nl, io.data(), root);
  if (c.mode == "blocked")
    return fa_reduce_blocked((fa_block_plan* const*)plans.data(), nl, io.data(), root);
  return fa_reduce_sharded((fa_shard_plan* const*)plans.data(), nl, io.data(), root);
}

void destroy_plan(const Case& c, void* p) {
  if (!p) return;
  if (c.mode == "multi" || c.mode == "multi_e1") {
    fa_multi_plan_destroy((fa_multi_plan*)p);
    return;
  }
  if (c.mode == "chained") fa_chain_plan_destroy((fa_chain_plan*)p);
  else if (c.mode == "striped") fa_stripe_plan_destroy((fa_stripe_plan*)p);
  else if (c.mode == "blocked") fa_block_plan_destroy((fa_block_plan*)p);
  else fa_shard_plan_destroy((fa_shard_plan*)p);
}

// The generator's client `client` into one slot's buckets, on stream st (the
// gaps between segments are never written: they stay as allocated).
int fill_slot(const Layout& L, float* d32, int64_t* d64, int client, int mode, hipStream_t st) {
  for (size_t k = 0; k < L.s32.size(); ++k) {
    const int rc = fa_synth_fill_f32(d32 + L.s32[k].offset, L.s32[k].numel,
                                     L.params ? L.key32[k] : (int)k, client,
                                     L.params ? L.mu[k] : 0.f, L.params ? L.sigma[k] : 0.05f,
                                     mode, st);
    if (rc) return rc;
  }
  for (size_t k = 0; k < L.s64.size(); ++k) {
    const int rc = fa_synth_fill_i64(d64 + L.s64[k].offset, L.s64[k].numel,
                                     L.params ? L.key64[k] : (int)(1000 + k), client, mode, st);
    if (rc) return rc;
  }
  return 0;
}

bool read_floats(const char* path, size_t count, std::vector<float>* out, std::string* err) {
  FILE* f = fopen(path, "rb");
  out->assign(count, 0.f);
  const size_t got = f ? fread(out->data(), 4, count, f) : 0;
  const bool more = f && fgetc(f) != EOF;
  if (f) fclose(f);
  if (got == count && !more) return true;
  *err = std::string(path) + ": expected " + std::to_string(count) + " float32";
  return false;
}

bool run_case(const Case& c, const Layout& L) {
  int n = 0;
  for (int k : c.counts) n += k;
  const int64_t F = L.f32_numel, I = std::max<int64_t>(L.i64_numel, 1);
  const int K = (int)c.rounds.size();
  auto refuse = [&](const std::string& what) {
    printf("{\"case\": \"%s\", \"ok\": false, \"error\": \"%s\"}\n", c.text.c_str(), what.c_str());
    return false;
  };
  // round 0 from files (special values), else the generator
  std::vector<float> file32, filew;
  std::string ferr;
  if (getenv("FA_LOOP_CLIENTS") &&
      !read_floats(getenv("FA_LOOP_CLIENTS"), (size_t)n * F, &file32, &ferr))
    return refuse(ferr);
  if (getenv("FA_LOOP_WEIGHTS") && !read_floats(getenv("FA_LOOP_WEIGHTS"), (size_t)n, &filew, &ferr))
    return refuse(ferr);

  // clients: the portable synthetic state; round k's slot i is client i + k * n
  std::vector<float*> c32(n);
  std::vector<int64_t*> c64(n);
  for (int i = 0; i < n; ++i) {
    HIPC(hipMalloc(&c32[i], F * 4));
    HIPC(hipMalloc(&c64[i], I * 8));
    HIPC(hipMemset(c32[i], 0, F * 4));
    HIPC(hipMemset(c64[i], 0, I * 8));
  }
  // (blocking: used before the ranks start and after they have finished)
  auto fill_all = [&](int k) {
    for (int i = 0; i < n; ++i) {
      if (fill_slot(L, c32[i], c64[i], i + k * n, c.data_mode, nullptr)) return false;
      if (k == 0 && !file32.empty())
        HIPC(hipMemcpy(c32[i], file32.data() + (size_t)i * F, F * 4, hipMemcpyHostToDevice));
    }
    return true;
  };
  // weights: host arrays, as the rounds read them; another vector every round
  std::vector<std::vector<float>> w(K, std::vector<float>(n));
  double ws = 0;
  for (int i = 0; i < n; ++i) ws += i + 1;
  for (int k = 0; k < K; ++k)
    for (int i = 0; i < n; ++i) w[k][i] = (float)(((i + 3 * k) % n + 1) / ws);
  if (!filew.empty()) w[0] = filew;

  // the single-GPU references, one per round, before any rank starts
  const bool exact = c.mode == "chained" || c.mode == "striped" || c.mode == "blocked" ||
                     c.mode == "multi" || c.mode == "mean_multi";
  const bool with64 = c.mode != "mean_multi";
  float* ref32;
  int64_t* ref64;
  HIPC(hipMalloc(&ref32, (size_t)K * F * 4));
  HIPC(hipMalloc(&ref64, (size_t)K * I * 8));
  HIPC(hipMemset(ref32, 0, (size_t)K * F * 4));
  HIPC(hipMemset(ref64, 0, (size_t)K * I * 8));
  fa_plan* rp = nullptr;
  const fa_seg* s64 = L.s64.empty() ? nullptr : L.s64.data();
  int rc = fa_plan_create(L.s32.data(), (int)L.s32.size(), F, s64, (int)L.s64.size(),
                          L.i64_numel, 0, FA_PLAN_GAPS_ARE_PADDING, &rp);
  // e1: the forward error bound 2N * 2^-24 * sum |w_i x_i| (/N for the mean)
  std::vector<std::vector<double>> bound(K);
  for (int k = 0; k < K && !rc; ++k) {
    if (!fill_all(k)) rc = -1;
    if (!rc)
      rc = fa_reduce(rp, (const float* const*)c32.data(), (const int64_t* const*)c64.data(), n,
                     c.rounds[k].weighted ? w[k].data() : nullptr, ref32 + (size_t)k * F,
                     ref64 + (size_t)k * I, 0, nullptr);
    HIPC(hipDeviceSynchronize());
    if (rc || exact) continue;
    bound[k].assign(F, 0.0);
    std::vector<float> x(F);
    for (int i = 0; i < n; ++i) {
      HIPC(hipMemcpy(x.data(), c32[i], F * 4, hipMemcpyDeviceToHost));
      const double wi = c.rounds[k].weighted ? (double)w[k][i] : 1.0 / n;
      for (int64_t e = 0; e < F; ++e) bound[k][e] += std::fabs((double)x[e]) * wi;
    }
    for (int64_t e = 0; e < F; ++e)
      bound[k][e] = bound[k][e] * 2.0 * n * std::ldexp(1.0, -24) + 1e-38;
  }
  if (!rc && K > 1 && !fill_all(0)) rc = -1;
  HIPC(hipDeviceSynchronize());
  if (rc) return refuse(std::string("reference: ") + fa_last_error());
  fa_plan_destroy(rp);

  // the ranks
  const int W = c.W;
  std::vector<Rank> R(W);
  int slot = 0;
  for (int r = 0; r < W; ++r) {
    bool result = false;
    for (const Round& rd : c.rounds) result = result || rd.root < 0 || rd.root == r;
    if (result) {
      HIPC(hipMalloc(&R[r].out32, F * 4));
      HIPC(hipMalloc(&R[r].out64, I * 8));
      HIPC(hipMalloc(&R[r].save32, (size_t)K * F * 4));
      HIPC(hipMalloc(&R[r].save64, (size_t)K * I * 8));
      HIPC(hipMemset(R[r].save32, 0xFF, (size_t)K * F * 4));
      HIPC(hipMemset(R[r].save64, 0xFF, (size_t)K * I * 8));
    }
    for (int j = 0; j < c.counts[r]; ++j) {
      R[r].c32.push_back(c32[slot + j]);
      R[r].c64.push_back(c64[slot + j]);
    }
    R[r].slot0 = slot;
    slot += c.counts[r];
  }
  // Round k on rank r, in three parts, all of them asynchronous on r's stream.
  // before: NaN-fill the result buckets (an unwritten element fails); the
  // round's arguments
  auto before = [&](Rank& k, int rd, fa_shard_io* io) {
    const int r = (int)(&k - R.data());
    const bool result = c.rounds[rd].root < 0 || c.rounds[rd].root == r;
    if (k.out32) {
      if (hipMemsetAsync(k.out32, 0xFF, F * 4, k.st) != hipSuccess ||
          hipMemsetAsync(k.out64, 0xFF, I * 8, k.st) != hipSuccess)
        return -1;
    }
    io->c32 = k.c32.data();
    io->c64 = L.s64.empty() ? nullptr : k.c64.data();
    io->weights = c.rounds[rd].weighted ? w[rd].data() + k.slot0 : nullptr;
    io->out32 = result ? k.out32 : nullptr;
    io->out64 = result ? k.out64 : nullptr;
    io->stream = k.st;
    return 0;
  };
  // after: keep the result, then overwrite the rank's own inputs in place with
  // the next round's
  const int gate_ms = getenv("FA_LOOP_GATE_MS") ? atoi(getenv("FA_LOOP_GATE_MS")) : 0;
  int clock_khz = 0;
  if (gate_ms > 0 &&
      hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeWallClockRate, 0) != hipSuccess)
    return refuse("no wall clock rate");
  if (gate_ms > 0 && (c.model != "threads" || gate_ms > 200))
    return refuse("FA_LOOP_GATE_MS: threads model only (its check runs between a rank's "
                  "rounds), at most 200");
  auto after = [&](Rank& k, int rd) {
    const int r = (int)(&k - R.data());
    if (c.rounds[rd].root < 0 || c.rounds[rd].root == r) {
      if (hipMemcpyAsync(k.save32 + (size_t)rd * F, k.out32, F * 4, hipMemcpyDeviceToDevice,
                         k.st) != hipSuccess ||
          hipMemcpyAsync(k.save64 + (size_t)rd * I, k.out64, I * 8, hipMemcpyDeviceToDevice,
                         k.st) != hipSuccess)
        return -1;
    }
    if (rd + 1 < K && gate_ms > 0) {
      if (!k.gate_end && hipEventCreateWithFlags(&k.gate_end, hipEventDisableTiming) != hipSuccess)
        return -1;
      hipLaunchKernelGGL(gate_kernel, dim3(1), dim3(1), 0, k.st, (long long)gate_ms * clock_khz,
                         (long long)gate_ms << 20);
      if (hipGetLastError() != hipSuccess || hipEventRecord(k.gate_end, k.st) != hipSuccess)
        return -1;
      k.gated = true;
    }
    if (rd + 1 < K)
      for (size_t j = 0; j < k.c32.size(); ++j)
        if (fill_slot(L, k.c32[j], k.c64[j], k.slot0 + (int)j + (rd + 1) * n, c.data_mode, k.st))
          return -1;
    return 0;
  };
  std::string err;
  bool failed = false;
  if (c.model == "threads") {
    unsigned char uid[FA_COMM_UID_BYTES];
    if (fa_comm_unique_id(uid, FA_COMM_UID_BYTES)) {
      err = fa_last_error();
      failed = true;
    } else {
      std::vector<std::thread> th;
      for (int r = 0; r < W; ++r)
        th.emplace_back([&, r] {
          Rank& k = R[r];
          (void)hipSetDevice(0);
          k.rc = fa_comm_init_rank(W, r, uid, FA_COMM_UID_BYTES, &k.comm);
          // the loopback pairs sends and receives on the host: never captured
          if (!k.rc) k.rc = fa_comm_set_graphs(k.comm, 0);
          const bool prof = getenv("FA_LOOP_PROFILE") && atoi(getenv("FA_LOOP_PROFILE"));
          if (!k.rc && prof) k.rc = fa_comm_set_profile(k.comm, 1);
          if (!k.rc) k.rc = create_plan(c, L, k);
          if (!k.rc) k.rc = hipStreamCreate(&k.st) == hipSuccess ? 0 : -1;
          for (int rd = 0; rd < K && !k.rc; ++rd) {
            std::vector<void*> plans{k.plan};
            std::vector<fa_shard_io> io(1);
            std::vector<Rank*> rk{&k};
            k.rc = before(k, rd, &io[0]);
            if (!k.rc) k.rc = run_round(c, L, c.rounds[rd].root, rk, plans, io);
            if (!k.rc && k.gated && hipEventQuery(k.gate_end) != hipErrorNotReady) {
              k.rc = -1;
              k.err = "round " + std::to_string(rd + 1) + ": gate too short / call blocked the host";
            }
            if (!k.rc) k.rc = after(k, rd);
          }
          if (!k.rc && prof && k.plan) {
            k.rc = fa_round_plan_profile(k.plan, &k.prof);
            k.has_prof = k.rc == 0;
          }
          if (k.rc && k.err.empty()) k.err = fa_last_error();
          if (k.st) (void)hipStreamSynchronize(k.st);
          if (k.gate_end) (void)hipEventDestroy(k.gate_end);
          k.gate_end = nullptr;
        });
      for (auto& t : th) t.join();
    }
  } else {
    std::vector<fa_comm*> comms(W, nullptr);
    std::vector<int> devs(W, 0);
    rc = fa_comm_init(W, devs.data(), comms.data());
    if (rc) {
      err = fa_last_error();
      failed = true;
    } else {
      std::vector<void*> plans(W);
      std::vector<fa_shard_io> io(W);
      std::vector<Rank*> rk(W);
      for (int r = 0; r < W && !failed; ++r) {
        R[r].comm = comms[r];
        R[r].rc = create_plan(c, L, R[r]);
        HIPC(hipStreamCreate(&R[r].st));
        plans[r] = R[r].plan;
        rk[r] = &R[r];
        if (R[r].rc) {
          R[r].err = fa_last_error();
          failed = true;
        }
      }
      for (int rd = 0; rd < K && !failed; ++rd) {
        rc = 0;
        for (int r = 0; r < W && !rc; ++r) rc = before(R[r], rd, &io[r]);
        if (!rc) rc = run_round(c, L, c.rounds[rd].root, rk, plans, io);
        for (int r = 0; r < W && !rc; ++r) rc = after(R[r], rd);
        if (rc) {
          err = fa_last_error();
          failed = true;
        }
      }
    }
  }
  HIPC(hipDeviceSynchronize());
  for (int r = 0; r < W; ++r)
    if (R[r].rc) {
      failed = true;
      if (err.empty()) err = "rank " + std::to_string(r) + ": " + R[r].err;
    }

  // the inputs: every client bucket still holds the last round's data
  unsigned long long* dbad = nullptr;
  unsigned long long bad_in = 0;
  if (!failed) {
    float* t32;
    int64_t* t64;
    HIPC(hipMalloc(&t32, F * 4));
    HIPC(hipMalloc(&t64, I * 8));
    HIPC(hipMalloc(&dbad, 8));
    HIPC(hipMemset(dbad, 0, 8));
    const bool from_file = K == 1 && !file32.empty();
    for (int i = 0; i < n; ++i) {
      if (fill_slot(L, t32, t64, i + (K - 1) * n, c.data_mode, nullptr)) {
        failed = true;
        err = fa_last_error();
        break;
      }
      if (from_file)
        HIPC(hipMemcpy(t32, file32.data() + (size_t)i * F, F * 4, hipMemcpyHostToDevice));
      for (const fa_seg& s : L.s32) count_diff(c32[i] + s.offset, t32 + s.offset, s.numel, dbad);
      for (const fa_seg& s : L.s64)
        count_diff(c64[i] + s.offset, t64 + s.offset, 2 * s.numel, dbad);
    }
    HIPC(hipMemcpy(&bad_in, dbad, 8, hipMemcpyDeviceToHost));
    (void)hipFree(t32);
    (void)hipFree(t64);
    (void)hipFree(dbad);
  }

  // compare, round by round
  std::vector<float> ref(F), got(F);
  std::vector<int64_t> ref_i(I), got_i(I);
  long long bad32 = 0, bad64 = 0, checked = 0;
  double worst = 0.0;
  int bad_round = 0;
  int64_t bad_first = -1, bad_last = -1;
  std::vector<char> round_ok(K, 1);
  std::string where;  // per failing round and rank: count, first / last bad element, unwritten
  const uint32_t kUnwritten = 0xFFFFFFFFu;
  for (int rd = 0; rd < K && !failed; ++rd) {
    HIPC(hipMemcpy(ref.data(), ref32 + (size_t)rd * F, F * 4, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(ref_i.data(), ref64 + (size_t)rd * I, I * 8, hipMemcpyDeviceToHost));
    checked = 0;
    for (int r = 0; r < W; ++r) {
      if (!(c.rounds[rd].root < 0 || c.rounds[rd].root == r)) continue;
      HIPC(hipMemcpy(got.data(), R[r].save32 + (size_t)rd * F, F * 4, hipMemcpyDeviceToHost));
      HIPC(hipMemcpy(got_i.data(), R[r].save64 + (size_t)rd * I, I * 8, hipMemcpyDeviceToHost));
      ++checked;
      long long rb = 0, rb64 = 0, nan = 0;
      int64_t first = -1, last = -1;
      for (const fa_seg& s : L.s32)
        for (int64_t e = s.offset; e < s.offset + s.numel; ++e) {
          uint32_t gb, fb;
          memcpy(&gb, &got[e], 4);
          memcpy(&fb, &ref[e], 4);
          bool b;
          if (exact) {
            // two NaNs are equal whatever their payload; the fill's own
            // pattern is an element the round did not write
            b = gb != fb && !(std::isnan(got[e]) && std::isnan(ref[e]) && gb != kUnwritten);
          } else {
            const double d = std::fabs((double)got[e] - (double)ref[e]);
            b = !(d <= bound[rd][e]);
            if (d / bound[rd][e] > worst) worst = d / bound[rd][e];
          }
          if (b) {
            ++rb;
            if (gb == kUnwritten) ++nan;
            if (first < 0) first = e;
            last = e;
          }
        }
      bad32 += rb;
      for (const fa_seg& s : L.s64)
        for (int64_t e = s.offset; e < s.offset + s.numel && with64; ++e)
          if (got_i[e] != ref_i[e]) ++rb64;
      bad64 += rb64;
      if (rb || rb64) {
        round_ok[rd] = 0;
        if (!bad_round) {
          bad_round = rd + 1;
          bad_first = first;
          bad_last = last;
        }
        where += "round " + std::to_string(rd + 1) + " rank " + std::to_string(r) + ": " +
                 std::to_string(rb) + " bad in [" + std::to_string(first) + ", " +
                 std::to_string(last) + "], " + std::to_string(nan) + " unwritten, " +
                 std::to_string(rb64) + " bad int64; ";
      }
      const char* dump = getenv("FA_LOOP_DUMP");
      if (dump && checked == 1 && rd == K - 1) {
        FILE* df = fopen(dump, "wb");
        if (df) {
          fwrite(got.data(), 4, (size_t)F, df);
          fwrite(got_i.data(), 8, (size_t)I, df);
          fclose(df);
        }
      }
    }
    if (!checked) round_ok[rd] = 0;
  }
  if (bad_in) where += std::to_string(bad_in) + " client words changed by the rounds; ";
  bool ok = !failed && bad32 == 0 && bad64 == 0 && bad_in == 0;
  for (char v : round_ok) ok = ok && v;
  if (err.empty()) err = where;
  if (err.size() > 1500) err = err.substr(0, 1500) + "...";
  char pbuf[256] = "null";
  if (R[0].has_prof)
    snprintf(pbuf, sizeof pbuf,
             "{\"exchange_us\": %.2f, \"comm_kernel_us\": %.2f, \"compute_kernel_us\": %.2f, "
             "\"wall_us\": %.2f, \"groups\": %d, \"kernels\": %d}",
             R[0].prof.exchange_us, R[0].prof.comm_kernel_us, R[0].prof.compute_kernel_us,
             R[0].prof.wall_us, R[0].prof.groups, R[0].prof.kernels);
  std::string oks = "[";
  for (int rd = 0; rd < K; ++rd)
    oks += std::string(rd ? ", " : "") + (round_ok[rd] && !failed ? "true" : "false");
  oks += "]";
  printf("{\"case\": \"%s\", \"ok\": %s, \"n\": %d, \"result_ranks\": %lld, \"bad_f32\": %lld, "
         "\"bad_i64\": %lld, \"check\": \"%s\", \"worst_err_over_bound\": %.4g, \"error\": \"%s\", "
         "\"profile\": %s, \"rounds\": %d, \"bad_round\": %d, \"bad_first\": %lld, "
         "\"bad_last\": %lld, \"round_ok\": %s, \"bad_inputs\": %llu}\n",
         c.text.c_str(), ok ? "true" : "false", n, checked, bad32, bad64,
         exact ? "bit-exact" : "error bound", worst, err.c_str(), pbuf, K, bad_round,
         (long long)bad_first, (long long)bad_last, oks.c_str(), bad_in);
  fflush(stdout);

  for (int r = 0; r < W; ++r) {
    destroy_plan(c, R[r].plan);
    if (R[r].st) (void)hipStreamDestroy(R[r].st);
    if (R[r].comm) fa_comm_destroy(R[r].comm);
    for (void* p : {(void*)R[r].out32, (void*)R[r].out64, (void*)R[r].save32, (void*)R[r].save64})
      if (p) (void)hipFree(p);
  }
  for (int i = 0; i < n; ++i) {
    (void)hipFree(c32[i]);
    (void)hipFree(c64[i]);
  }
  (void)hipFree(ref32);
  (void)hipFree(ref64);
  return ok;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: loop_round LAYOUT CASE...\n");
    return 2;
  }
  Layout L;
  if (!read_layout(argv[1], &L)) {
    fprintf(stderr, "bad layout file %s\n", argv[1]);
    return 2;
  }
  int fails = 0;
  for (int a = 2; a < argc; ++a) {
    Case c;
    if (!parse_case(argv[a], &c)) {
      fprintf(stderr, "bad case %s\n", argv[a]);
      return 2;
    }
    if (!run_case(c, L)) ++fails;
  }
  return fails ? 1 : 0;
}
